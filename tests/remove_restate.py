"""Plain-Python restatement of GraphAndTreeIndex::remove (lib/NGT/Index.h:1386-1455):
the duplicate search, DVPTree::remove / replace on the leaf (Tree.h:178-202,
Node.cpp:229-280) and NeighborhoodGraph::removeEdgesReliably built with
NGT_FORCED_REMOVE (Graph.cpp:641-864).  Distances come from the oracle
comparator of tests/oracle_py.py.  Test infrastructure only."""
import bisect
import ctypes

import numpy as np

import oracle_py as O


def erase_reverse_edge(lst, dist, id_):
    """Graph.cpp:705-736: the reverse edge is looked up by lower_bound on
    (stored distance, id) and erased only when the element there has the id."""
    p = bisect.bisect_left(lst, (dist, id_))
    if p < len(lst) and lst[p][1] == id_:
        del lst[p]
        return True
    return False


def insert_edge(lst, dist, id_):
    """Graph.cpp:762-805: insert at the lower_bound position unless the
    element there already has the id."""
    p = bisect.bisect_left(lst, (dist, id_))
    if p == len(lst) or lst[p][1] != id_:
        lst.insert(p, (dist, id_))
        return True
    return False


def relink_chain(metric, rows, nbr):
    """Graph.cpp:739-845: [(id at position i, id of the first strict minimum
    among later positions, distance)] for i = 0 .. d-2, the minimum swapped to
    position i + 1 after each step."""
    order = [int(v) for v in nbr]
    links = []
    for i in range(len(order) - 1):
        d = O.distances(metric, rows, rows[order[i]], order[i + 1:])
        m = int(np.argmin(d))  # the first minimum, as `d < mind` keeps it
        minj = i + 1 + m
        links.append((order[i], order[minj], np.float32(d[m])))
        order[i + 1], order[minj] = order[minj], order[i + 1]
    return links


class Index:
    def __init__(self, metric, rows, valid, offsets, ids, dists, tree, leaves, edge_size_for_search=0):
        self.metric = metric
        self.rows = rows
        self.valid = np.array(valid, dtype=np.uint8)
        n = len(offsets) - 1
        self.lists = [[(float(dists[e]), int(ids[e])) for e in range(int(offsets[v]), int(offsets[v + 1]))]
                      for v in range(n)]
        self.has_node = [bool(v and v < len(self.valid) and self.valid[v]) for v in range(n)]
        self.tree = tree
        self.leaves = [list(l) for l in leaves]
        self.es = edge_size_for_search
        self.message = ""

    def csr(self):
        offs = np.zeros(len(self.lists) + 1, np.uint64)
        offs[1:] = np.cumsum([len(l) for l in self.lists])
        ids = np.array([e[1] for l in self.lists for e in l], np.uint32)
        dists = np.array([e[0] for l in self.lists for e in l], np.float32)
        return offs, ids, dists

    def leaf_of(self, id_):
        t = self.tree
        if t["root"] & 0x80000000:
            return t["root"] & 0x7FFFFFFF
        q = np.ascontiguousarray(self.rows[id_])
        piv = np.ascontiguousarray(t["in_pivot"])
        child = np.ascontiguousarray(t["in_child"], dtype=np.uint32)
        border = np.ascontiguousarray(t["in_border"], dtype=np.float32)
        nd = np.zeros(1, np.uint64)
        leaf = O.lib().ngto_tree_leaf(O.METRICS[self.metric], 2 if piv.dtype == np.float32 else 1, q.ctypes.data,
                                      piv.shape[1], t["root"], piv.ctypes.data, piv.strides[0],
                                      O._p(child, ctypes.c_uint32), O._p(border, ctypes.c_float), 5,
                                      O._p(nd, ctypes.c_uint64))
        return leaf & 0x7FFFFFFF

    def _evaluated_edges_exist(self, v):
        lst = self.lists[v]
        for _, t in lst[:len(lst) if self.es <= 0 else self.es]:
            if t >= len(self.valid) or not self.valid[t]:
                self.message = "get: Not in-memory or invalid offset of node. idx=%d size=%d" % (t, len(self.valid))
                return False
        return True

    def remove(self, id_):
        """True when removed; a refusal leaves everything as it was."""
        if id_ <= 0 or id_ >= len(self.valid) or not self.valid[id_]:
            self.message = "get: Not in-memory or invalid offset of node. idx=%d size=%d" % (id_, len(self.valid))
            return False
        if id_ >= len(self.has_node) or not self.has_node[id_]:
            self.valid[id_] = 0
            return True
        if not self._evaluated_edges_exist(id_):
            return False
        offs, ids, _ = self.csr()
        found, _, _ = O.search(self.metric, self.rows, offs, ids, self.rows[id_], [id_], 2, np.float32(0.1),
                               radius=0.0, edge_size=max(self.es, 0))
        if len(found) == 0:
            self.message = "Not found the specified id"
            return False
        replace = 0
        if len(found) > 1:
            replace = int(found[1]) if int(found[0]) == id_ else int(found[0])
            if not self._evaluated_edges_exist(replace):
                return False
        leaf = self.leaves[self.leaf_of(id_)]
        if replace:
            if id_ in leaf:
                leaf[leaf.index(id_)] = replace
        else:
            if id_ not in leaf:
                self.message = "remove:: cannot remove from tree. id=%d" % id_
                return False
            leaf.remove(id_)
        self.remove_edges_reliably(id_)
        self.valid[id_] = 0
        return True

    def remove_edges_reliably(self, id_):
        node = [e for e in self.lists[id_] if e[1] != id_]
        for dist, nb in node:
            erase_reverse_edge(self.lists[nb], dist, id_)
        for a, b, d in relink_chain(self.metric, self.rows, [e[1] for e in node]):
            insert_edge(self.lists[a], float(d), b)
            insert_edge(self.lists[b], float(d), a)
        self.lists[id_] = []
        self.has_node[id_] = False
