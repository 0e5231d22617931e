"""The filter rule of the uint8 Cosine / Angle matrix-core scan on the CPU
(ngt_amd/csrc/scan_u8cos_bound.h: an integer triple (s, na, nb) the float
filter rejects finishes strictly above the k-th distance).
tests/cxx/scan_u8cos_bound_host.cpp holds the checks; this module compiles and
runs it, plain and under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_u8cos_filter_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "scan_u8cos_bound_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + list(flags) +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "scan_u8cos_bound_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"thresholds (\d+) probes (\d+) rejected (\d+) failures (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    thresholds, probes, rejected, failures = (int(g) for g in m.groups())
    # 2 metrics x (~16,000 strided + 5 x up to 129 dense) kd x 144 norm pairs x up to 15 steps; about half rejected
    assert failures == 0 and thresholds > 2 * 16000 and probes > 500 * thresholds and rejected > probes // 4
