"""Plain-Python restatement of the reference's refine-anng
(GraphReconstructor::refineANNG, GraphReconstructor.h:803-924; addEdge,
Graph.h:845-873) -- the second checker of the device implementation
(ngt_amd/csrc/refine.cpp).

A graph is a list indexed by node id (slot 0 the dummy) of lists of
``(id, distance)`` with ``distance`` the stored float32 widened (exactly) to a
Python float, as in onng_restate.py.  The list steps compare stored values
only; the full loop takes its searches from the CPU oracle (tree seeds plus
graph search).  Test infrastructure only.
"""
import bisect

import numpy as np

from onng_restate import _key, from_csr, to_csr  # noqa: F401  (re-exported)

INT_MAX = 2 ** 31 - 1


def outgoing(node, nid, results):
    """Step 2 for one node: append the results other than the node itself,
    std::sort by (distance, id), erase every element whose id equals its
    predecessor's (adjacent repeats only)."""
    lst = sorted(list(node) + [r for r in results if r[0] != nid], key=_key)
    out = []
    prev = 0
    for e in lst:
        if e[0] == prev:
            continue
        out.append(e)
        prev = e[0]
    return out


def add_edge(node, nid, dist):
    """GraphIndex::addEdge(node, id, distance, identityCheck=false): lower_bound
    of (distance, id); nothing if that position holds the same id, else insert.
    -> whether the edge went in."""
    keys = [_key(e) for e in node]
    p = bisect.bisect_left(keys, (dist, nid))
    if p < len(node) and node[p][0] == nid:
        return False
    node.insert(p, (nid, dist))
    return True


def merge(graph, first, results, incoming, stats=None):
    """Steps 2 and 3 of one batch, in place.  results[q]: the result list of
    node first + q in result order; queries past the last row are ignored.
    `stats`, when a dict, counts under "incoming_at_a_present_distance" the
    incoming edges that went into a list already holding their distance."""
    n = len(graph)
    results = results[:max(0, n - first)]
    for q, res in enumerate(results):
        graph[first + q] = outgoing(graph[first + q], first + q, res)
    if not incoming:
        return graph
    for q, res in enumerate(results):
        for rid, dist in res:
            if rid != first + q:
                tie = stats is not None and any(e[1] == dist for e in graph[rid])
                if add_edge(graph[rid], first + q, dist) and tie:
                    stats["incoming_at_a_present_distance"] = stats.get("incoming_at_a_present_distance", 0) + 1
    return graph


def prune(graph, k):
    """Step 4: every list longer than k is cut to k."""
    for v in range(1, len(graph)):
        if len(graph[v]) > k:
            del graph[v][k:]
    return graph


def merge_csr(offsets, ids, dists, first, res_ids, res_dists, res_counts, incoming):
    """merge() on a CSR graph and a padded block of results [count][stride]."""
    g = from_csr(offsets, ids, dists)
    rd = np.asarray(res_dists, np.float32).astype(np.float64)
    results = [[(int(res_ids[q][j]), float(rd[q][j])) for j in range(int(res_counts[q]))]
               for q in range(len(res_counts))]
    return to_csr(merge(g, first, results, incoming))


def prune_csr(offsets, ids, dists, k):
    return to_csr(prune(from_csr(offsets, ids, dists), k))


def edge_size(prop, explore, epsilon):
    """NeighborhoodGraph::getEdgeSize (Graph.h:675-692); explore None = not given."""
    es = int(prop["EdgeSizeForSearch"]) if explore is None or explore == -1 else int(explore)
    if es == 0:
        return INT_MAX
    if es > 0:
        return es
    if es == -2:
        coef = float(np.float32(float(np.float32(epsilon)) + 1.0))
        add = 10.0 ** ((coef - 1.0) * float(np.float32(int(prop["DynamicEdgeSizeRate"]))))
        return INT_MAX if add >= INT_MAX else int(int(prop["DynamicEdgeSizeBase"]) + add)
    raise ValueError("NGT::getEdgeSize: Invalid edge size parameters %d:%s" % (es, prop["EdgeSizeForSearch"]))


def refine(rows, tree, prop, offsets, ids, dists, epsilon, num_edges=0, explore=None, batch_size=10000, threads=8,
           metric="l2", valid=None, stats=None):
    """The whole refinement of an index under `metric`; returns the new CSR.
    `rows` are the stored rows (float32 or uint8, normalised already where the
    metric normalises): refineANNG searches with the stored objects themselves.
    valid[v] == 0 is a removed row: ObjectRepository::isEmpty skips its search
    and its outgoing step, and it has no results to hand out."""
    import oracle_py as O
    graph = from_csr(offsets, ids, dists)
    n = len(graph)
    creation = int(prop["EdgeSizeForCreation"])
    size = -num_edges if num_edges < 0 else max(num_edges, creation)
    es = edge_size(prop, explore, epsilon)
    seed_size = int(prop["SeedSize"])
    for bid in range(1, n, batch_size):
        batch = [v for v in range(bid, min(bid + batch_size, n)) if valid is None or valid[v]]
        results = [[] for _ in range(min(bid + batch_size, n) - bid)]
        if batch:
            off, eid, _ = to_csr(graph)
            seeds = [O.tree_seeds(metric, tree, rows[v], size, seed_size, rows.dtype)[0] for v in batch]
            ri, rd, rn, _ = O.search_batch(metric, rows, off, eid, rows[batch], seeds, size, np.float32(epsilon),
                                           edge_size=es, threads=threads)
            rd = rd.astype(np.float64)
            for q, v in enumerate(batch):
                results[v - bid] = [(int(ri[q, j]), float(rd[q, j])) for j in range(int(rn[q]))]
        merge(graph, bid, results, num_edges == 0, stats)
    if num_edges > 0:
        prune(graph, num_edges)
    return to_csr(graph)
