#!/usr/bin/env python3
"""Exact scan of a float L1 index (ngt_amd_linear_search_device): two builds
of the library, alternating in child processes on one device -- identical
ids, distance bits and counts required -- and their times with the spread,
one JSON line per k.  With NGT_AMD_TEST_KNOBS=1 NGT_AMD_SCAN_STATS=1 in the
environment the filtered scan also prints its candidates per query and part
(stderr), to hold against k ln(rows per part / k).
usage: scan_l1f_timing.py OTHER_LIB [n] [nq] [dim] [rounds] [reps] [k ...]
  OTHER_LIB: a libngt_amd.so to compare this tree's build with (a build of
  the parent commit).  Rows and queries are uniform in [0, 1)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(n, nq, dim, k, reps, lib, out):
    # plain ctypes: the other build may lack entry points the package declares
    import ctypes
    from ctypes import byref, c_double, c_int, c_uint32, c_uint64, c_void_p

    import torch
    from ngt_amd.device import DISTANCE
    L = ctypes.CDLL(lib)
    L.ngt_amd_last_error.restype = ctypes.c_char_p
    L.ngt_amd_index_create.argtypes = [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_uint32]
    L.ngt_amd_index_set_objects_device.argtypes = [c_void_p, c_void_p, c_uint64]
    L.ngt_amd_linear_search_device.argtypes = [c_void_p, c_void_p, c_uint64, c_uint32, c_uint32, c_double, c_void_p,
                                               c_void_p, c_void_p, c_void_p]
    L.ngt_amd_last_scan_kernel.argtypes = [c_void_p]

    def chk(rc):
        if rc:
            raise RuntimeError(L.ngt_amd_last_error().decode())

    dev = torch.device("cuda:0")
    dp = (dim + 15) // 16 * 16
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    rows = torch.zeros((n + 1, dp), dtype=torch.float32, device=dev)
    rows[1:, :dim] = torch.rand((n, dim), dtype=torch.float32, device=dev, generator=g)
    q = torch.zeros((nq, dp), dtype=torch.float32, device=dev)
    q[:, :dim] = torch.rand((nq, dim), dtype=torch.float32, device=dev, generator=g)
    h = c_void_p()
    chk(L.ngt_amd_index_create(byref(h), 0, DISTANCE["l1"], 2, dim))
    chk(L.ngt_amd_index_set_objects_device(h, rows.data_ptr(), n + 1))
    oi = torch.zeros((nq, k), dtype=torch.int32, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    on = torch.zeros((nq,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    times = []
    for rep in range(reps + 1):  # the first call warms up (code objects, buffers, the rows' image)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        chk(L.ngt_amd_linear_search_device(h, q.data_ptr(), dp * 4, nq, k, -1.0, oi.data_ptr(), od.data_ptr(),
                                           on.data_ptr(), st.cuda_stream))
        e1.record(st)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    np.savez(out, ids=oi.cpu().numpy(), d=od.cpu().numpy(), n=on.cpu().numpy(), ms=np.array(times[1:]),
             kernel=L.ngt_amd_last_scan_kernel(h))


def compare(libs, n, nq, dim, k, rounds, reps, tmp):
    ms = {name: [] for name in libs}
    kernel, first, same = {}, None, True
    for r in range(rounds):
        for name, path in libs.items():
            out = os.path.join(tmp, "k%d_%s.npz" % (k, name))
            subprocess.check_call([sys.executable, __file__, "--child"] + [str(x) for x in (n, nq, dim, k, reps)] +
                                  [path, out], timeout=600)
            a = np.load(out)
            ms[name] += a["ms"].tolist()
            kernel[name] = int(a["kernel"])
            if first is None:
                first = a
            same = same and (np.array_equal(a["n"], first["n"]) and np.array_equal(a["ids"], first["ids"]) and
                             np.array_equal(a["d"].view(np.uint32), first["d"].view(np.uint32)))
    line = {"metric": "l1", "n": n, "nq": nq, "dim": dim, "k": k, "identical": bool(same)}
    for name in libs:
        v = np.array(ms[name])
        line[name] = {"kernel": kernel[name], "ms": [round(x, 3) for x in v], "median_ms": float(np.median(v)),
                      "min_ms": float(v.min()), "max_ms": float(v.max())}
    print(json.dumps(line), flush=True)
    return same


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        run(*[int(x) for x in sys.argv[2:7]], sys.argv[7], sys.argv[8])
        sys.exit(0)
    other = os.path.abspath(sys.argv[1])
    args = sys.argv[2:] + ["1000000", "10000", "128", "3", "3"][len(sys.argv) - 2:]
    n, nq, dim, rounds, reps = [int(x) for x in args[:5]]
    ks = [int(x) for x in args[5:]] or [10, 16]
    libs = {"other": other, "this": os.path.join(ROOT, "ngt_amd", "libngt_amd.so")}
    with tempfile.TemporaryDirectory() as tmp:
        ok = [compare(libs, n, nq, dim, k, rounds, reps, tmp) for k in ks]
    sys.exit(0 if all(ok) else 1)
