"""ONNG reconstruction on the device: ``ngt_amd_onng_reconstruct`` of
include/ngt_amd.h (edge and path adjustment of GraphOptimizer::execute) on a
host CSR graph."""
import ctypes

import numpy as np

from . import NativeError, _sigs, last_error, lib


def fast_path_capacity():
    """Longest list the one-wave sort and the LDS id table take."""
    return int(lib().ngt_amd_onng_fast_path_capacity())


def reconstruct(offsets, ids, dists, outgoing, incoming, path_adjustment, min_edges=0, input_is_anng=True,
                device=0, with_stats=False):
    """Returns the new (offsets uint64, ids uint32, dists float32); with
    ``with_stats`` also the stage times and counters as a dict."""
    L = lib()
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    i = np.ascontiguousarray(ids, dtype=np.uint32)
    d = np.ascontiguousarray(dists, dtype=np.float32)
    if len(off) < 1 or len(i) != len(d) or int(off[-1]) != len(i):
        raise NativeError("onng.reconstruct: offsets, ids and dists do not describe one CSR graph")
    p = _sigs.OnngParams(int(outgoing), int(incoming), int(bool(path_adjustment)), int(bool(input_is_anng)),
                         int(min_edges))
    ne = ctypes.c_uint64(0)
    if L.ngt_amd_onng_reconstruct(int(device), off.ctypes.data, i.ctypes.data, d.ctypes.data, len(off) - 1,
                                  ctypes.byref(p), ctypes.byref(ne)):
        raise NativeError(last_error())
    o2 = np.zeros(len(off), np.uint64)
    i2 = np.zeros(ne.value, np.uint32)
    d2 = np.zeros(ne.value, np.float32)
    if L.ngt_amd_onng_get_graph(o2.ctypes.data, i2.ctypes.data, d2.ctypes.data):
        raise NativeError(last_error())
    if not with_stats:
        return o2, i2, d2
    st = _sigs.OnngStats()
    if L.ngt_amd_onng_last_stats(ctypes.byref(st)):
        raise NativeError(last_error())
    return o2, i2, d2, {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}
