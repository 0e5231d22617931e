"""The scalar rules of the float L1 byte-SAD filtered scan on the CPU
(ngt_amd/csrc/scan_l1f_bound.h: the quantiser, the error bounds E_x and e_q
and the integer threshold T -- a pair with SAD > T + E_x has a comparator
distance strictly above kd).  tests/cxx/scan_l1f_bound_host.cpp holds the
checks; this module compiles and runs it, plain and under the address and
undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_l1f_bound_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "scan_l1f_bound_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + list(flags) +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "scan_l1f_bound_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"thresholds (\d+) pairs (\d+) rejected (\d+) failures (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    thresholds, pairs, rejected, failures = (int(g) for g in m.groups())
    # 3000 tables x 24 rows x 24 k-th distances.  Half the tables have queries inside the rows' range, and at
    # most half of their (row, k-th) pairs lie above the k-th distance: a working filter rejects a good part of
    # that quarter, a vacuous one nothing
    assert failures == 0 and thresholds > 400000 and pairs == 3000 * 24 * 24 and rejected > pairs // 10
