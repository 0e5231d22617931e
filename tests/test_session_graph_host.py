"""The list rules of a build session on the CPU (ngt_amd/csrc/session_graph.h:
the four insertion rules, the sorted addEdge, addEdgeDeletingExcessEdges,
getRandomSeeds, the host half of removal, the adjacency rows, the CSR form)
against a model restated from the reference's text by another method, and the
generator against the C library's rand().  tests/cxx/session_graph_host.cpp
holds the directed cases and the differential run; this module compiles and
runs it, plain and under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngt_amd", "csrc")


def build_host_program(exe, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "session_graph_host.cpp")])


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_graph_rules_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "session_graph_host")
    build_host_program(exe, flags)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"sequences (\d+) operations (\d+) checks (\d+) failures (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    sequences, operations, checks, failures = (int(g) for g in m.groups())
    assert failures == 0
    assert sequences >= 400 and operations >= 400 * 64 and checks > operations


def test_the_host_program_includes_only_the_header():
    src = open(os.path.join(ROOT, "tests", "cxx", "session_graph_host.cpp")).read()
    project = [i for i in re.findall(r'#include "([^"]+)"', src)]
    assert project == ["../../ngt_amd/csrc/session_graph.h"]
    header = open(os.path.join(CSRC, "session_graph.h")).read()
    assert "hip" not in " ".join(re.findall(r"#include [<\"]([^>\"]+)[>\"]", header))


def test_the_rules_are_stated_once():
    """build.cpp and ngt_amd_api.cpp take the rules from the header and define none of them themselves."""
    for name in ("build.cpp", "ngt_amd_api.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "session_graph.h"' in text, name
        for fn in ("od_less", "add_edge", "add_edge_deleting_excess", "get_random_seeds"):
            assert not re.search(r"\b(?:bool|int|void|std::string)\s+%s\s*\(" % fn, text), (name, fn)
        # a getRandomSeeds loop of its own: the draw's arithmetic
        assert "RAND_MAX" not in text and "2147483647" not in text, name
        assert not re.search(r"\+\s*1\.0\s*\)\s*/", text), name


def test_one_dispatch_table_for_the_stored_types():
    for name in ("build_kernels.hip", "remove_kernels.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "stored_dispatch.h"' in text, name
        assert "NGT_BUILD_DISPATCH" not in text and "NGT_REMOVE_DISPATCH" not in text, name
        assert not re.search(r"#define\s+NGT_\w*DISPATCH", text), name
    header = open(os.path.join(CSRC, "stored_dispatch.h")).read()
    assert len(re.findall(r"#define\s+NGT_STORED_DISPATCH\b", header)) == 1
