"""The order-deciding arithmetic of a DVP-tree leaf split on the CPU
(ngt_amd/csrc/build_order.h, the bodies ngt_tree_insert_kernel runs): std_sort
against the machine's std::sort on tie-heavy keys, the depth-limit heap sort
included, and pivot_variance against a long double variance and the documented
lane order.  tests/cxx/build_order_host.cpp holds the cases; this module
compiles and runs it, plain and under the address and undefined-behaviour
sanitizers (the 64-entry explicit stack, the `first - 1` reads of the unguarded
loops)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_program(exe, extra=()):
    # -ffp-contract=off: the fma calls are the only fused operations, as in the kernel's build
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-DNGT_BUILD_ORDER_COUNT"] + list(extra) +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "build_order_host.cpp")])


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_sort_and_variance_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "build_order_host")
    build_host_program(exe, flags)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"sort_cases (\d+) heap_sorts (-?\d+) variance_cases (\d+) worst_error_over_bound (\S+) failures (\d+)",
                  r.stdout)
    assert m, r.stdout[-2000:]
    sort_cases, heap_sorts, variance_cases, failures = int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(5))
    assert failures == 0
    # every n in 2..101 and 128 in every key class; every n in 1..101 in every value class
    assert sort_cases >= 101 * 30 and variance_cases >= 101 * 30
    assert heap_sorts > 0, "no input reached introsort's depth limit"
    assert float(m.group(4)) <= 1.0


def test_the_kernel_file_takes_the_functions_from_the_header():
    """One statement of each function: the kernel file includes the header and defines none of them itself."""
    kernel = open(os.path.join(ROOT, "ngt_amd", "csrc", "build_kernels.hip")).read()
    assert '#include "build_order.h"' in kernel
    for name in ("pivot_variance", "std_sort", "heap_sort", "unguarded_partition", "insertion_sort"):
        assert not re.search(r"\b(?:void|double|SortItem\*)\s+%s\s*\(" % name, kernel), name
