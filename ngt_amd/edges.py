"""Edge-count optimisation on the device: ``ngt_amd_recut_anng`` of
include/ngt_amd.h (GraphReconstructor::reconstructANNGFromANNG) on a host CSR
graph.  ``DeviceIndex.optimize_edges`` (device.py) runs the whole procedure."""
import ctypes

from . import NativeError, last_error, lib
from ._csr import as_csr, take_graph


def recut(offsets, ids, dists, K, device=0):
    """The graph re-cut to K edges: the new (offsets uint64, ids uint32, dists float32)."""
    L = lib()
    off, i, d = as_csr(offsets, ids, dists, "edges.recut", 1)
    ne = ctypes.c_uint64(0)
    if L.ngt_amd_recut_anng(int(device), off.ctypes.data, i.ctypes.data, d.ctypes.data, len(off) - 1, int(K),
                            ctypes.byref(ne)):
        raise NativeError(last_error())
    return take_graph(L.ngt_amd_recut_get_graph, len(off) - 1, ne.value)
