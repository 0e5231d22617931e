"""The two scalar rules of the uint8 L2 matrix-core scan on the CPU
(ngt_amd/csrc/scan_u8_bound.h: the float distance of an integer sum and
max_sum_for_distance, its inverse), exhaustively over every sum in [0, 2^24).
tests/cxx/scan_u8_bound_host.cpp holds the checks; this module compiles and
runs it, plain and under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_sum_bounds_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "scan_u8_bound_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + list(flags) +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "scan_u8_bound_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"sums (\d+) distances (\d+) failures (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    sums, distances, failures = (int(g) for g in m.groups())
    assert failures == 0 and sums == 1 << 24 and distances > 1 << 22
