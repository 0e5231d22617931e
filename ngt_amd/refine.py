"""refine-anng on the device: the ``ngt_amd_refine_*`` entry points of
include/ngt_amd.h (GraphReconstructor::refineANNG) on host CSR graphs and on a
``DeviceIndex``."""
import ctypes

import numpy as np

from . import NativeError, _sigs, last_error, lib
from ._csr import as_csr, take_graph


def fast_path_capacity():
    """Longest list the one-wave sort takes; longer ones are sorted in global memory."""
    return int(lib().ngt_amd_refine_fast_path_capacity())


def _result(nrows, nedges, with_stats):
    L = lib()
    o2, i2, d2 = take_graph(L.ngt_amd_refine_get_graph, nrows, nedges)
    if not with_stats:
        return o2, i2, d2
    st = _sigs.RefineStats()
    if L.ngt_amd_refine_last_stats(ctypes.byref(st)):
        raise NativeError(last_error())
    return o2, i2, d2, {k: getattr(st, k) for k, _ in st._fields_}


def merge(offsets, ids, dists, first_id, res_ids, res_dists, res_counts, incoming, device=0, with_stats=False):
    """The outgoing step (and the incoming step when ``incoming``) for one block
    of results: query q is node first_id + q with results res_ids/res_dists[q,
    :res_counts[q]].  Returns the new (offsets uint64, ids uint32, dists float32)."""
    off, i, d = as_csr(offsets, ids, dists, "refine.merge", 2)
    ri = np.ascontiguousarray(res_ids, dtype=np.uint32)
    rd = np.ascontiguousarray(res_dists, dtype=np.float32)
    rn = np.ascontiguousarray(res_counts, dtype=np.uint32)
    if ri.ndim != 2 or ri.shape != rd.shape or ri.shape[0] != len(rn):
        raise NativeError("refine.merge: res_ids and res_dists are [count][stride], res_counts [count]")
    ne = ctypes.c_uint64(0)
    if lib().ngt_amd_refine_merge(int(device), off.ctypes.data, i.ctypes.data, d.ctypes.data, len(off) - 1,
                                  int(first_id), ri.shape[0], ri.shape[1], ri.ctypes.data, rd.ctypes.data,
                                  rn.ctypes.data, int(bool(incoming)), ctypes.byref(ne)):
        raise NativeError(last_error())
    return _result(len(off) - 1, ne.value, with_stats)


def prune(offsets, ids, dists, num_edges, device=0):
    """Every list longer than num_edges cut to num_edges."""
    off, i, d = as_csr(offsets, ids, dists, "refine.prune", 2)
    ne = ctypes.c_uint64(0)
    if lib().ngt_amd_refine_prune(int(device), off.ctypes.data, i.ctypes.data, d.ctypes.data, len(off) - 1,
                                  int(num_edges), ctypes.byref(ne)):
        raise NativeError(last_error())
    return _result(len(off) - 1, ne.value, False)


def refine_anng(index, offsets, ids, dists, epsilon, num_edges, edge_size_for_creation, explore_edge_size=-1,
                batch_size=10000, with_stats=False):
    """The whole refinement on a ``DeviceIndex`` that has rows and a tree;
    offsets/ids/dists is its graph with distances.  Afterwards the index
    searches the refined graph, which is returned."""
    off, i, d = as_csr(offsets, ids, dists, "refine.refine_anng", 2)
    p = _sigs.RefineParams(float(epsilon), int(num_edges), int(explore_edge_size), int(batch_size),
                           int(edge_size_for_creation), 0)
    ne = ctypes.c_uint64(0)
    if lib().ngt_amd_refine_anng(index.h, off.ctypes.data, i.ctypes.data, d.ctypes.data, len(off) - 1,
                                 ctypes.byref(p), ctypes.byref(ne)):
        raise NativeError(last_error())
    return _result(len(off) - 1, ne.value, with_stats)
