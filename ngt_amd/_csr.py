"""A host CSR graph with distances on its way into and out of the graph stages
(onng.py, refine.py, edges.py)."""
import numpy as np

from . import NativeError, last_error


def as_csr(offsets, ids, dists, who, min_len):
    """(offsets uint64, ids uint32, dists float32), contiguous; ``offsets`` holds
    at least ``min_len`` entries and ends at the number of ids."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    i = np.ascontiguousarray(ids, dtype=np.uint32)
    d = np.ascontiguousarray(dists, dtype=np.float32)
    if len(off) < min_len or len(i) != len(d) or int(off[-1]) != len(i):
        raise NativeError("%s: offsets, ids and dists do not describe one CSR graph" % who)
    return off, i, d


def take_graph(getter, nrows, nedges):
    """The graph a stage left on this thread, through its ``*_get_graph``."""
    off = np.zeros(nrows + 1, np.uint64)
    i = np.zeros(nedges, np.uint32)
    d = np.zeros(nedges, np.float32)
    if getter(off.ctypes.data, i.ctypes.data, d.ctypes.data):
        raise NativeError(last_error())
    return off, i, d
