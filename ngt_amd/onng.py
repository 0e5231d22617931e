"""ONNG reconstruction on the device: ``ngt_amd_onng_reconstruct`` of
include/ngt_amd.h (edge and path adjustment of GraphOptimizer::execute) on a
host CSR graph."""
import ctypes

from . import NativeError, _sigs, last_error, lib
from ._csr import as_csr, take_graph


def fast_path_capacity():
    """Longest list the one-wave sort and the LDS id table take."""
    return int(lib().ngt_amd_onng_fast_path_capacity())


def reconstruct(offsets, ids, dists, outgoing, incoming, path_adjustment, min_edges=0, input_is_anng=True,
                device=0, with_stats=False):
    """Returns the new (offsets uint64, ids uint32, dists float32); with
    ``with_stats`` also the stage times and counters as a dict."""
    L = lib()
    off, i, d = as_csr(offsets, ids, dists, "onng.reconstruct", 1)
    p = _sigs.OnngParams(int(outgoing), int(incoming), int(bool(path_adjustment)), int(bool(input_is_anng)),
                         int(min_edges))
    ne = ctypes.c_uint64(0)
    if L.ngt_amd_onng_reconstruct(int(device), off.ctypes.data, i.ctypes.data, d.ctypes.data, len(off) - 1,
                                  ctypes.byref(p), ctypes.byref(ne)):
        raise NativeError(last_error())
    o2, i2, d2 = take_graph(L.ngt_amd_onng_get_graph, len(off) - 1, ne.value)
    if not with_stats:
        return o2, i2, d2
    st = _sigs.OnngStats()
    if L.ngt_amd_onng_last_stats(ctypes.byref(st)):
        raise NativeError(last_error())
    return o2, i2, d2, {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}
