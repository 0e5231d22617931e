"""Edge-count optimisation on the device: ``ngt_amd_recut_anng`` of
include/ngt_amd.h (GraphReconstructor::reconstructANNGFromANNG) on a host CSR
graph.  ``DeviceIndex.optimize_edges`` (device.py) runs the whole procedure."""
import ctypes

import numpy as np

from . import NativeError, last_error, lib


def recut(offsets, ids, dists, K, device=0):
    """The graph re-cut to K edges: the new (offsets uint64, ids uint32, dists float32)."""
    L = lib()
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    i = np.ascontiguousarray(ids, dtype=np.uint32)
    d = np.ascontiguousarray(dists, dtype=np.float32)
    if len(off) < 1 or len(i) != len(d) or int(off[-1]) != len(i):
        raise NativeError("edges.recut: offsets, ids and dists do not describe one CSR graph")
    ne = ctypes.c_uint64(0)
    if L.ngt_amd_recut_anng(int(device), off.ctypes.data, i.ctypes.data, d.ctypes.data, len(off) - 1, int(K),
                            ctypes.byref(ne)):
        raise NativeError(last_error())
    o2 = np.zeros(len(off), np.uint64)
    i2 = np.zeros(ne.value, np.uint32)
    d2 = np.zeros(ne.value, np.float32)
    if L.ngt_amd_recut_get_graph(o2.ctypes.data, i2.ctypes.data, d2.ctypes.data):
        raise NativeError(last_error())
    return o2, i2, d2
