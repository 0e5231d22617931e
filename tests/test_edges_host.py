"""CPU-side checks of the edge-count optimisation (ngt optimize-#-of-edges): the
pure host unit (ngt_amd/csrc/edge_optimizer.cpp) through
tests/cxx/edge_optimizer_host.cpp, plain and under ASan/UBSan; the numpy
restatement of the graph re-cut (tests/edges_data.py), which checks the kernel
in tests/test_gpu_edges.py, on a graph small enough to write its result out;
and the two refusals of the C API that are decided before any device work,
against the reference's text (tests/golden/edge_optimization.json)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import edges_data as D
import ngt_amd
from ngt_amd import _sigs, base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLD, "edge_optimization.json")))
REF_NGT = os.path.join(ROOT, "oracle", "_ref", "ngt")
PREFIX = "Capi : ngt_optimize_number_of_edges() : Error: "


# ---- the pure host unit, without Python in the loop -----------------------------
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_host_unit(tmp_path, flags):
    exe = str(tmp_path / "edge_optimizer_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + list(flags) +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "edge_optimizer_host.cpp"),
                           os.path.join(ROOT, "ngt_amd", "csrc", "edge_optimizer.cpp"),
                           os.path.join(ROOT, "ngt_amd", "csrc", "accuracy_table.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: ")


# ---- the restatement of the re-cut ----------------------------------------------
def csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    ids, ds = [], []
    for v, l in enumerate(lists):
        ids += [m for m, _ in l]
        ds += [d for _, d in l]
        off[v + 1] = len(ids)
    return off, np.array(ids, np.uint32), np.array(ds, np.float32)


def lists_of(off, ids, ds):
    return [[(int(ids[e]), float(ds[e])) for e in range(int(off[v]), int(off[v + 1]))] for v in range(len(off) - 1)]


# Slot 0 is the dummy.  Node 5 lists a higher id before its lower ones; node 6's
# third distance is below its second, which ends its walk there; node 7's three
# distances tie, so ids alone order them.
EIGHT = [
    [],
    [(2, 1.0), (3, 2.0)],
    [(1, 1.0), (4, 1.5), (3, 3.0)],
    [(1, 2.0), (2, 3.0), (4, 3.5)],
    [(2, 1.5), (3, 3.5), (1, 4.0)],
    [(6, 0.5), (4, 1.0), (1, 2.5), (2, 2.5), (3, 6.0)],
    [(5, 0.5), (1, 2.0), (2, 1.0), (3, 5.0)],
    [(2, 0.25), (6, 0.25), (5, 0.25)],
]


def test_restatement_on_a_graph_written_out():
    off, ids, ds = csr(EIGHT)
    # K = 1: every node keeps its first lower-id entry, in both directions
    assert lists_of(*D.recut(off, ids, ds, 1)) == [
        [],
        [(2, 1.0), (3, 2.0)],                 # from 2 and 3
        [(7, 0.25), (1, 1.0), (4, 1.5)],      # from 7, own, from 4
        [(1, 2.0)],
        [(5, 1.0), (2, 1.5)],                 # from 5 (6 is higher and not counted), own
        [(6, 0.5), (4, 1.0)],
        [(5, 0.5)],
        [(2, 0.25)],
    ]
    # K = 2
    assert lists_of(*D.recut(off, ids, ds, 2)) == [
        [],
        [(2, 1.0), (3, 2.0), (6, 2.0), (5, 2.5)],
        [(7, 0.25), (1, 1.0), (4, 1.5), (3, 3.0)],
        [(1, 2.0), (2, 3.0), (4, 3.5)],
        [(5, 1.0), (2, 1.5), (3, 3.5)],
        [(6, 0.5), (4, 1.0), (1, 2.5)],
        [(7, 0.25), (5, 0.5), (1, 2.0)],
        [(2, 0.25), (6, 0.25)],
    ]
    # K above every list: all lower-id entries before a walk's end (6's ends at (2, 1.0) < 2.0)
    assert lists_of(*D.recut(off, ids, ds, 100)) == [
        [],
        [(2, 1.0), (3, 2.0), (6, 2.0), (5, 2.5), (4, 4.0)],
        [(7, 0.25), (1, 1.0), (4, 1.5), (5, 2.5), (3, 3.0)],
        [(1, 2.0), (2, 3.0), (4, 3.5), (5, 6.0)],
        [(5, 1.0), (2, 1.5), (3, 3.5), (1, 4.0)],
        [(7, 0.25), (6, 0.5), (4, 1.0), (1, 2.5), (2, 2.5), (3, 6.0)],
        [(7, 0.25), (5, 0.5), (1, 2.0)],
        [(2, 0.25), (5, 0.25), (6, 0.25)],
    ]


def test_restatement_keeps_repeats_that_are_not_adjacent():
    # node 3 lists 1 twice: in 1's list 2 stands between the two copies of 3, so both stay; in 3's own
    # list the copies of 1 are neighbours and the second goes
    lists = [[], [], [(1, 2.0)], [(1, 1.0), (1, 3.0)]]
    assert lists_of(*D.recut(*csr(lists), 5)) == [[], [(3, 1.0), (2, 2.0), (3, 3.0)], [(1, 2.0)], [(1, 1.0)]]
    lists = [[], [], [], [(1, 1.0), (1, 1.0), (2, 1.0)]]
    assert lists_of(*D.recut(*csr(lists), 5)) == [[], [(3, 1.0)], [(3, 1.0)], [(1, 1.0), (2, 1.0)]]


# ---- refusals that need no device ----------------------------------------------
def snapshot(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_default_parameter():
    p = ngt_amd.lib().ngt_get_anng_edge_optimization_parameter()
    assert (p.no_of_queries, p.no_of_results, p.no_of_threads, p.target_no_of_objects, p.no_of_sample_objects,
            p.max_of_no_of_edges, p.log) == (200, 50, 16, 0, 100000, 100, False)
    assert p.target_accuracy == np.float32(0.9)


@pytest.fixture(scope="module")
def small_index(tmp_path_factory):
    return D.make_index(str(tmp_path_factory.mktemp("edges") / "u8_3000"), "u8_3000")


def test_saved_index_is_the_reference_created_one(small_index):
    assert open(os.path.join(small_index, "prf")).read() == CASES["X1"]["prf"]


@pytest.mark.skipif(not os.path.exists(REF_NGT), reason="the reference CLI (oracle/_ref/ngt) is not built")
def test_recipe_reproduces_the_refusals(small_index, tmp_path):
    """The two quick cases of the fixture recipe (the others take the reference 5-17 s of CPU
    time each, three times over), and the claim the tests rest on: the objects appended through
    the C API and saved are the obj file `ngt create` writes."""
    import make_edge_optimization_goldens as M
    out = M.run_recipe(REF_NGT, str(tmp_path), cases=[c for c in M.CASES if c[0] in ("X1", "X2")])
    assert out == {name: CASES[name] for name in ("X1", "X2")}
    assert open(os.path.join(small_index, "obj"), "rb").read() == open(str(tmp_path / "u8_3000" / "obj"), "rb").read()


@pytest.mark.parametrize("name", ["X1", "X2"])
def test_refusals_before_any_device_work(name, small_index):
    L = ngt_amd.lib()
    before = snapshot(small_index)
    err = L.ngt_create_error_object()
    assert not L.ngt_optimize_number_of_edges(small_index.encode(), D.parameter(CASES[name]["args"]), err)
    assert base._err_string(L, err) == PREFIX + CASES[name]["error"]
    edge, acc = ctypes.c_size_t(7), ctypes.c_float(7.0)
    assert not L.ngt_optimize_number_of_edges_with_result(small_index.encode(), D.parameter(CASES[name]["args"]),
                                                          ctypes.byref(edge), ctypes.byref(acc), err)
    assert base._err_string(L, err) == PREFIX + CASES[name]["error"]
    assert (edge.value, acc.value) == (7, 7.0)
    L.ngt_destroy_error_object(err)
    assert snapshot(small_index) == before


def test_null_path_and_missing_index(tmp_path):
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    p = L.ngt_get_anng_edge_optimization_parameter()
    assert not L.ngt_optimize_number_of_edges(None, p, err)
    assert base._err_string(L, err) == "Capi : ngt_optimize_number_of_edges() : parametor error: index path = 0"
    assert not L.ngt_optimize_number_of_edges(str(tmp_path / "nothing").encode(), p, err)
    assert base._err_string(L, err).startswith(PREFIX)
    L.ngt_destroy_error_object(err)


def test_the_timing_driven_stub_stays():
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    opt = L.ngt_create_optimizer(True, err)
    assert not L.ngt_optimizer_adjust_search_coefficients(opt, b"x", err)
    assert "not implemented in the MI355X build yet" in base._err_string(L, err)
    L.ngt_destroy_optimizer(opt)
    L.ngt_destroy_error_object(err)


def test_signature_structs_match_the_header():
    # ngt_amd_edge_sample: 4 x 8 + 4 x 4 + 32 x 8 + 32 x 8 + 3 x 8 bytes
    assert ctypes.sizeof(_sigs.EdgeSample) == 32 + 16 + 256 + 256 + 24
    assert ctypes.sizeof(_sigs.EdgeParams) == 3 * 8 + 8 + 3 * 8 + ctypes.sizeof(_sigs.BuildParams)
