#!/usr/bin/env python3
"""Exact scan of a float L1 index with lists of 17 .. 128 results
(ngt_amd_linear_search_device): two builds of the library, alternating in
fresh child processes on one device -- identical ids, distance bits and counts
required -- and their times with the spread, one JSON line per k.
usage: scan_l1fwide_timing.py OTHER_LIB [n] [nq] [dim] [rounds] [reps] [k ...]
  OTHER_LIB: a libngt_amd.so to compare this tree's build with (a build of
  the parent commit).  This tree's build runs with NGT_AMD_LINEAR_L1FWIDE=1
  (and the knobs' master switch), the other one with the knob removed: its
  float L1 batches of more than 16 results take the quad-per-row kernel.
  Rows and queries are uniform in [0, 1).
With NGT_AMD_SCAN_STATS=1 in the environment this tree's scan also prints its
candidates and rounds per query and part (stderr), to hold against
k ln(rows per part / k); the counters are atomics, so such a run is no timing.
Every child runs under its own time limit; the first failure ends the run."""
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
            env = {v: x for v, x in os.environ.items() if v != "NGT_AMD_LINEAR_L1FWIDE"}
            if name == "this":
                env.update(NGT_AMD_TEST_KNOBS="1", NGT_AMD_LINEAR_L1FWIDE="1")
            # a child that faults, aborts or runs out of time raises here: nothing more starts on the device
            subprocess.check_call(["timeout", "-k", "10", "240", sys.executable, __file__, "--child"] +
                                  [str(x) for x in (n, nq, dim, k, reps)] + [path, out], env=env)
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
    # the criterion of DESIGN.md 4a: this build's slowest call below the other's fastest
    line["slowest_below_fastest"] = line["this"]["max_ms"] < line["other"]["min_ms"]
    print(json.dumps(line), flush=True)
    return same


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        run(*[int(x) for x in sys.argv[2:7]], sys.argv[7], sys.argv[8])
        sys.exit(0)
    other = os.path.abspath(sys.argv[1])
    args = sys.argv[2:] + ["1000000", "10000", "128", "3", "3"][len(sys.argv) - 2:]
    n, nq, dim, rounds, reps = [int(x) for x in args[:5]]
    ks = [int(x) for x in args[5:]] or [17, 100]
    libs = {"other": other, "this": os.path.join(ROOT, "ngt_amd", "libngt_amd.so")}
    with tempfile.TemporaryDirectory() as tmp:
        for k in ks:
            if not compare(libs, n, nq, dim, k, rounds, reps, tmp):
                sys.exit(1)
