#!/usr/bin/env python3
"""Exact scan of a float index under Normalized Cosine, Normalized Angle and
Angle (ngt_amd_linear_search_device), k = 10 and k = 100: two builds of the
library, alternating in child processes on one device -- identical ids,
distance bits and counts required -- and their times with the spread, one JSON
line per shape.
usage: scan_dot_timing.py OTHER_LIB [n] [nq] [dim] [rounds] [reps]
  OTHER_LIB: a libngt_amd.so to compare this tree's build with (a build of
  the parent commit).
Rows and queries are unit vectors.  "on" says whether this build's median is
below the other's by more than both spreads (max - min)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(m, k) for m in ("normalized_cosine", "normalized_angle", "angle") for k in (10, 100)]


def run(metric, n, nq, dim, k, reps, lib, out):
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

    def unit_rows(m):
        x = torch.rand((m, dim), dtype=torch.float32, device=dev, generator=g) - 0.5
        return x / x.norm(dim=1, keepdim=True)

    rows = torch.zeros((n + 1, dp), dtype=torch.float32, device=dev)
    rows[1:, :dim] = unit_rows(n)
    q = torch.zeros((nq, dp), dtype=torch.float32, device=dev)
    q[:, :dim] = unit_rows(nq)
    h = c_void_p()
    chk(L.ngt_amd_index_create(byref(h), 0, DISTANCE[metric], 2, dim))
    chk(L.ngt_amd_index_set_objects_device(h, rows.data_ptr(), n + 1))
    oi = torch.zeros((nq, k), dtype=torch.int32, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    on = torch.zeros((nq,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    times = []
    for rep in range(reps + 1):  # the first call warms up (code objects, the rows' bf16 image)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        chk(L.ngt_amd_linear_search_device(h, q.data_ptr(), dp * 4, nq, k, -1.0, oi.data_ptr(), od.data_ptr(),
                                           on.data_ptr(), st.cuda_stream))
        e1.record(st)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    np.savez(out, ids=oi.cpu().numpy(), d=od.cpu().numpy(), n=on.cpu().numpy(), ms=np.array(times[1:]),
             kernel=L.ngt_amd_last_scan_kernel(h))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    if sys.argv[1] == "--child":
        run(sys.argv[2], *[int(x) for x in sys.argv[3:8]], sys.argv[8], sys.argv[9])
        sys.exit(0)
    other = os.path.abspath(sys.argv[1])
    args = sys.argv[2:] + ["1000000", "10000", "128", "3", "3"][len(sys.argv) - 2:]
    n, nq, dim, rounds, reps = [int(x) for x in args[:5]]
    libs = {"other": other, "this": os.path.join(ROOT, "ngt_amd", "libngt_amd.so")}
    all_same = True
    for metric, k in SHAPES:
        ms = {name: [] for name in libs}
        kernel, first, same = {}, None, True
        for r in range(rounds):
            for name, path in libs.items():
                out = "/tmp/scan_dot_timing_%s.npz" % name
                subprocess.run([sys.executable, __file__, "--child", metric] + [str(x) for x in (n, nq, dim, k, reps)] +
                               [path, out], timeout=600, check=True)
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
        t, o = line["this"], line["other"]
        line["on"] = bool(same and o["median_ms"] - t["median_ms"] >
                          max(o["max_ms"] - o["min_ms"], t["max_ms"] - t["min_ms"]))
        print(json.dumps(line), flush=True)
        all_same = all_same and same
    sys.exit(0 if all_same else 1)
