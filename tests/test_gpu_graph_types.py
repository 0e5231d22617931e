"""KNNG, IANNG and ONNG construction on the device: every case of
tests/graph_type_data.py, built through the C API (ngt_batch_append_index,
ngt_create_index, ngt_save_index), against the files the reference's `ngt
create -g k|i|o` wrote for the same rows (tests/golden/gtype_<type>_<case>/,
make_graph_type_goldens.py).  grp and tre are compared byte for byte; a
mismatch is reported as the first graph node, leaf or internal node that
differs.  tests/test_graph_type_goldens.py holds what each fixture has to contain."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import build_data as D
import graph_type_data as G
import ngt_files as F
import oracle_py as O
from ngt_amd import base
from test_gpu_build_matrix import first_graph_difference, first_tree_difference, read

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PRF_KEYS = ("GraphType", "OutgoingEdge", "IncomingEdge")


def assert_same_files(out, case):
    dim = D.CASES[case["data"]][2]
    for f in ("grp", "tre"):
        got, want = os.path.join(out, f), os.path.join(GOLD, case["dir"], f)
        if read(got) == read(want):
            continue
        if f == "grp":
            pytest.fail("%s grp: %s" % (case["dir"], first_graph_difference(got, want)))
        pytest.fail("%s tre: %s" % (case["dir"], first_tree_difference(got, want, dim, G.dtype_of(case))))
    got, want = F.read_prf(os.path.join(out, "prf")), F.read_prf(os.path.join(GOLD, case["dir"], "prf"))
    for k in PRF_KEYS:
        assert got[k] == want[k], (case["dir"], k)


@pytest.mark.parametrize("case", G.CASES, ids=[c["dir"] for c in G.CASES])
def test_device_build_equals_the_reference_files(tmp_path, case):
    """The incremental case goes through two ngt_create_index calls."""
    rows, _ = D.dataset(case["data"])
    out = G.build_index(str(tmp_path / case["dir"]), case, rows)
    assert_same_files(out, case)


@pytest.mark.parametrize("batch", [2000, 64])
def test_knng_does_not_depend_on_the_batch_size(tmp_path, batch):
    """The lists are exact and the tree takes the objects in id order, so one
    batch of all rows and batches of 64 give the files of batches of 200
    (BatchSizeForCreation itself is a prf key outside the comparison)."""
    case = G.BY_DIR["gtype_knng_l2_f20"]
    rows, _ = D.dataset(case["data"])
    out = G.build_index(str(tmp_path / "knng"), case, rows, batch=batch)
    assert_same_files(out, case)


def test_knng_on_duplicates_beyond_the_edge_count(tmp_path):
    """l1_f_dups holds one row 150 times: from the twelfth copy on, an object is
    not among its own E + 1 nearest by (distance, id), and the debug build of
    the reference asserts in ObjectDistances::moveFrom.  Its release build goes
    on, and so does this one: the list is the E + 1 smallest (distance, id),
    minus the object itself if it is there, else minus the smallest -- restated
    here over the oracle's exact linear search."""
    case = G._case("k", "l1_f_dups")
    data, _ = D.dataset("l1_f_dups")
    out = G.build_index(str(tmp_path / "dups"), case, data)
    offs, ids, ds = F.read_grp(os.path.join(out, "grp"))
    rows = np.zeros((len(data) + 1, 16), np.float32)
    rows[1:] = data
    E = case["edges"]
    wi, wd, wn = O.linear_search_batch("l1", rows, rows[1:], E + 1)
    second_branch = []
    for v in range(1, len(rows)):
        assert wn[v - 1] == E + 1
        li, ld = wi[v - 1].tolist(), wd[v - 1]
        at = li.index(v) if v in li else 0
        if v not in li:
            second_branch.append(v)
        keep = [j for j in range(E + 1) if j != at]
        a, b = int(offs[v]), int(offs[v + 1])
        assert ids[a:b].tolist() == [li[j] for j in keep], v
        assert ds[a:b].tobytes() == ld[keep].tobytes(), v
    assert 912 in second_branch


@pytest.mark.parametrize("name", ["gtype_knng_l2_f20", "gtype_ianng_l1_u8_ties", "gtype_onng_ham_u8"])
def test_live_handle_answers_like_the_saved_index(tmp_path, name):
    case = G.BY_DIR[name]
    rows, _ = D.dataset(case["data"])
    q = np.ascontiguousarray(D.queries(case["data"])[:8], dtype=np.float32)
    path = str(tmp_path / name)
    L, live, err = G.build_index(path, case, rows, keep_open=True)
    try:
        ids, ds, n = np.zeros((8, 10), np.uint32), np.zeros((8, 10), np.float32), np.zeros(8, np.uint32)
        assert L.ngt_batch_search_index(live, q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 8, q.shape[1], 10,
                                        0.1, -1.0, -1, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                        ds.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                        n.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), err), base._err_string(L, err)
    finally:
        L.ngt_close_index(live)
        L.ngt_destroy_error_object(err)
    saved = base.Index(path)
    try:
        wi, wd, wn = saved.batch_search(q, 10, 0.1)
    finally:
        saved.close()
    assert n.tolist() == wn.tolist() and int(n.min()) > 0
    for i in range(8):
        assert ids[i, :n[i]].tolist() == wi[i, :n[i]].tolist(), i
        assert ds[i, :n[i]].tobytes() == wd[i, :n[i]].tobytes(), i


def test_cxx_property_graph_type_builds_the_knng_fixture(tmp_path):
    """NGT::Property::graphType = GraphTypeKNNG, NGT::Index::create, append,
    createIndex(1) and save (tests/cxx/graph_type_sample.cpp)."""
    case = G.BY_DIR["gtype_knng_l2_f20"]
    exe = str(tmp_path / "graph_type_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "graph_type_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
    rows, otype = D.dataset(case["data"])
    data = str(tmp_path / "rows.tsv")
    D.write_text(rows, otype, data)
    idx = str(tmp_path / "knng_cxx")
    r = subprocess.run([exe, idx, data, "20"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "objects 2000"
    assert_same_files(idx, case)
