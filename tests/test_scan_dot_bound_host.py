"""The threshold rules of the dot-family matrix-core scan on the CPU
(ngt_amd/csrc/scan_dot_bound.h: T(kd) for Normalized Cosine, Normalized L2,
Normalized Angle and Angle -- every dot product or cosine below it finishes
strictly above kd).  tests/cxx/scan_dot_bound_host.cpp holds the checks; this
module compiles and runs it, plain and under the address and
undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_dot_thresholds_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "scan_dot_bound_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + list(flags) +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "scan_dot_bound_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"thresholds (\d+) probes (\d+) failures (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    thresholds, probes, failures = (int(g) for g in m.groups())
    # 4 metrics x (130,276 strided + 6 x up to 129 dense) kd; most of them below the top: 64 probes each
    assert failures == 0 and thresholds > 4 * 130000 and probes > 16 * thresholds
