#!/usr/bin/env python3
"""Exact scan of a uint8 L1 / Hamming index with rows of 272 .. 1024 padded
bytes (ngt_amd_linear_search_device): two builds of the library, alternating
in child processes on one device -- identical ids, distance bits and counts
required -- and their times with the spread.
usage: scan_byteslong_timing.py OTHER_LIB [metric] [k] [n] [nq] [dim] [rounds] [reps]
  OTHER_LIB: a libngt_amd.so to compare this tree's build with (a build of
  the parent commit).  This tree's build runs with NGT_AMD_LINEAR_BYTESLONG=1
  (and the knobs' master switch), the other one with the knob removed: its
  batches on such rows take the quad-per-row kernel.
  metric: l1 or hamming, random bytes.
Every child runs under its own time limit; the first failure ends the run."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(metric, k, n, nq, dim, reps, lib, out):
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
    rows = torch.zeros((n + 1, dp), dtype=torch.uint8, device=dev)
    for lo in range(1, n + 1, 65536):  # a slab of rows at a time
        part = rows[lo:lo + 65536, :dim]
        part.copy_(torch.randint(0, 256, part.shape, dtype=torch.uint8, device=dev, generator=g))
    q = torch.zeros((nq, dp), dtype=torch.uint8, device=dev)
    q[:, :dim].copy_(torch.randint(0, 256, (nq, dim), dtype=torch.uint8, device=dev, generator=g))
    h = c_void_p()
    chk(L.ngt_amd_index_create(byref(h), 0, DISTANCE[metric], 1, dim))
    chk(L.ngt_amd_index_set_objects_device(h, rows.data_ptr(), n + 1))
    oi = torch.zeros((nq, k), dtype=torch.int32, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    on = torch.zeros((nq,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    times = []
    for rep in range(reps + 1):  # the first call warms up (code objects, the context's buffers)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        chk(L.ngt_amd_linear_search_device(h, q.data_ptr(), dp, nq, k, -1.0, oi.data_ptr(), od.data_ptr(),
                                           on.data_ptr(), st.cuda_stream))
        e1.record(st)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    np.savez(out, ids=oi.cpu().numpy(), d=od.cpu().numpy(), n=on.cpu().numpy(), ms=np.array(times[1:]),
             kernel=L.ngt_amd_last_scan_kernel(h))


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        run(sys.argv[2], *[int(x) for x in sys.argv[3:8]], sys.argv[8], sys.argv[9])
        sys.exit(0)
    other = os.path.abspath(sys.argv[1])
    args = sys.argv[2:] + ["l1", "10", "1000000", "10000", "512", "3", "3"][len(sys.argv) - 2:]
    metric = args[0]
    k, n, nq, dim, rounds, reps = [int(x) for x in args[1:7]]
    libs = {"other": other, "this": os.path.join(ROOT, "ngt_amd", "libngt_amd.so")}
    ms = {name: [] for name in libs}
    kernel, first, same = {}, None, True
    for r in range(rounds):
        for name, path in libs.items():
            out = "/tmp/scan_byteslong_timing_%s.npz" % name
            env = {v: x for v, x in os.environ.items() if v != "NGT_AMD_LINEAR_BYTESLONG"}
            if name == "this":
                env.update(NGT_AMD_TEST_KNOBS="1", NGT_AMD_LINEAR_BYTESLONG="1")
            # a child that faults, aborts or runs out of time raises here: nothing more starts on the device
            subprocess.check_call(["timeout", "-k", "10", "240", sys.executable, __file__, "--child", metric] +
                                  [str(x) for x in (k, n, nq, dim, reps)] + [path, out], env=env)
            a = np.load(out)
            ms[name] += a["ms"].tolist()
            kernel[name] = int(a["kernel"])
            if first is None:
                first = a
            same = same and (np.array_equal(a["n"], first["n"]) and np.array_equal(a["ids"], first["ids"]) and
                             np.array_equal(a["d"].view(np.uint32), first["d"].view(np.uint32)))
    line = {"metric": metric, "n": n, "nq": nq, "dim": dim, "k": k, "identical": bool(same)}
    for name in libs:
        v = np.array(ms[name])
        line[name] = {"kernel": kernel[name], "ms": [round(x, 3) for x in v], "median_ms": float(np.median(v)),
                      "min_ms": float(v.min()), "max_ms": float(v.max())}
    print(json.dumps(line), flush=True)
    sys.exit(0 if same else 1)
