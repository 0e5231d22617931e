#!/usr/bin/env python3
"""Exact scan of a float index with lists of more than 16 results
(ngt_amd_linear_search_device): two builds of the library, alternating in
child processes on one device -- identical ids, distance bits and counts
required -- and their times with the spread, one JSON line per shape.
usage: scan_wide_timing.py OTHER_LIB [n] [nq] [dim] [rounds] [reps]
  OTHER_LIB: a libngt_amd.so to compare this tree's build with (a build of
  the parent commit).
Shapes: L2 at k = 100, 32 and 17, Cosine at k = 100.  At k = 100 one more run
of this build with NGT_AMD_SCAN_STATS prints the kernel's candidate and round
counts next to k ln(rows per part / k) per query and part."""
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [("l2", 100), ("l2", 32), ("l2", 17), ("cosine", 100)]


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
    kernel = L.ngt_amd_last_scan_kernel(h) if hasattr(L, "ngt_amd_last_scan_kernel") else -1
    np.savez(out, ids=oi.cpu().numpy(), d=od.cpu().numpy(), n=on.cpu().numpy(), ms=np.array(times[1:]), kernel=kernel,
             cus=torch.cuda.get_device_properties(dev).multi_processor_count)


def child(metric, n, nq, dim, k, reps, lib, out, env=None):
    return subprocess.run([sys.executable, __file__, "--child", metric] + [str(x) for x in (n, nq, dim, k, reps)] +
                          [lib, out], timeout=600, check=True, env=env, stderr=subprocess.PIPE, text=True).stderr


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
                out = "/tmp/scan_wide_timing_%s.npz" % name
                child(metric, n, nq, dim, k, reps, path, out)
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
        if k == 100:
            err = child(metric, n, nq, dim, k, 0, libs["this"], "/tmp/scan_wide_timing_stats.npz",
                        dict(os.environ, NGT_AMD_TEST_KNOBS="1", NGT_AMD_SCAN_STATS="1"))
            line["stats"] = [s for s in err.splitlines() if s.startswith("scan_mfma")][-1:]
            # the library's split: one workgroup per CU, no more parts than 256-row tiles
            parts = min(max(1, int(a["cus"]) // ((nq + 127) // 128)), (n + 1 + 255) // 256)
            line["parts"] = parts
            line["k_ln_rows_per_part_over_k"] = round(k * math.log(n / parts / k))
        print(json.dumps(line), flush=True)
        all_same = all_same and same
    sys.exit(0 if all_same else 1)
