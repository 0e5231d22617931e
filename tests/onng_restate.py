"""Plain-Python restatement of the reference's ONNG reconstruction
(GraphReconstructor.h:33-63 extractGraph, :389-423 convertToANNG, :425-561
reconstructGraph, :197-386 adjustPathsEffectively) -- the second checker of
the device implementation (ngt_amd/csrc/onng.cpp).

A graph is a list indexed by node id (slot 0 the dummy) of lists of
``(id, distance)`` with ``distance`` the stored float32 widened (exactly) to a
Python float; every comparison is on those stored values and no distance is
recomputed.  Test infrastructure only.
"""
import numpy as np


def from_csr(offsets, ids, dists):
    il = np.asarray(ids).tolist()
    dl = np.asarray(dists, np.float32).astype(np.float64).tolist()   # exact
    ol = np.asarray(offsets).tolist()
    return [list(zip(il[ol[v]:ol[v + 1]], dl[ol[v]:ol[v + 1]])) for v in range(len(ol) - 1)]


def to_csr(graph):
    offsets = np.zeros(len(graph) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(l) for l in graph])
    ids = np.array([e[0] for l in graph for e in l], np.uint32)
    dists = np.array([e[1] for l in graph for e in l], np.float32)
    return offsets, ids, dists


def _key(e):
    # ObjectDistance::operator< (Common.h:1946-1959): distance, then id
    return (e[1], e[0])


def sort_unique(lst):
    """std::sort by (distance, id), then drop every entry whose id equals the
    previously kept entry's id (prev starts at 0)."""
    out = []
    prev = 0
    for e in sorted(lst, key=_key):
        if e[0] == prev:
            continue
        out.append(e)
        prev = e[0]
    return out


def convert_to_anng(graph):
    g = [list(l) for l in graph]
    for v in range(1, len(graph)):
        for (u, d) in graph[v]:
            g[u].append((v, d))
    return [sort_unique(l) for l in g]


def edge_adjustment(graph, stored, o, i):
    """reconstructGraph(graph, out, o, i): `stored` are the node lists as they
    are on disk (what a node with fewer than o entries keeps)."""
    out = []
    for v in range(len(graph)):
        if o == 0:
            out.append([])
        elif len(graph[v]) >= o:
            out.append(list(graph[v][:o]))
        else:
            out.append(list(stored[v]))
    for v in range(1, len(graph)):
        for (u, d) in graph[v][:i]:
            out[u].append((v, d))
    return [sort_unique(l) for l in out]


class RepeatedId(Exception):
    pass


def path_adjustment(tmp, min_edges=0, stats=None):
    """adjustPathsEffectively(out, minE) as a closed-form rule; `stats`, when a
    dict, receives the static dependency depth: the longest chain of same-rank
    references p < v that a rank-synchronous evaluation has to resolve."""
    n = len(tmp)
    rank_of = []
    for v in range(n):
        if any(_key(a) > _key(b) for a, b in zip(tmp[v], tmp[v][1:])):
            raise ValueError("list of node %d is not in (distance, id) order" % v)
        m = {}
        for r, (u, _) in enumerate(tmp[v]):
            if u in m:
                raise RepeatedId(v)
            m[u] = r
        rank_of.append(m)
    # every (p, rank of dst in p) that could prove a path for the edge tmp[v][r]
    cand = [[[] for _ in l] for l in tmp]
    for v in range(1, n):
        mine = rank_of[v]
        for (p, dp) in tmp[v]:
            for dst in mine.keys() & rank_of[p].keys():
                dd = tmp[v][mine[dst]][1]
                rp = rank_of[p][dst]
                if dp < dd and tmp[p][rp][1] < dd:
                    cand[v][mine[dst]].append((p, rp))
    kept = [set() for _ in range(n)]          # ids currently in out[v]
    out = [[] for _ in range(n)]
    depth_max = 0
    maxlen = max([len(l) for l in tmp] or [0])
    alive = [v for v in range(1, n) if tmp[v]]
    for r in range(maxlen):
        depth = {}
        alive = [v for v in alive if r < len(tmp[v])]
        for v in alive:                       # ascending id
            dst, dd = tmp[v][r]
            drop = False
            dep = 0
            if len(out[v]) + len(tmp[v]) - r > min_edges:
                for (p, rp) in cand[v][r]:
                    if p not in kept[v]:
                        continue
                    if rp == r and p < v:
                        dep = max(dep, depth.get(p, 0) + 1)
                    if dst in kept[p]:        # out[p] as it is now: p's rank-r decision only if p < v
                        drop = True
            depth[v] = dep
            depth_max = max(depth_max, dep)
            if not drop:
                out[v].append((dst, dd))
                kept[v].add(dst)
    if stats is not None:
        stats["depth"] = depth_max
    return [sorted(l, key=_key) for l in out]


def reconstruct(offsets, ids, dists, outgoing, incoming, path_adjustment_on, min_edges=0, input_is_anng=True):
    """GraphOptimizer::execute's graph stages on a CSR; returns the new CSR."""
    stored = from_csr(offsets, ids, dists)
    out = stored
    if outgoing > 0 or incoming > 0:
        graph = stored if input_is_anng else convert_to_anng(stored)
        out = edge_adjustment(graph, stored, outgoing, incoming)
    if path_adjustment_on:
        out = path_adjustment(out, min_edges)
    return to_csr(out)
