"""CPU-side checks of refine-anng: the plain-Python restatement
(tests/refine_restate.py) against the reference-built fixtures
(tests/golden/refine1k), the fixture recipe, the argument checks of
`ngt_refine_anng` that need no device, the C++ header and the ngtpy signature
(no device call is made here)."""
import filecmp
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ngt_amd
import refine_data as D
import refine_restate as R
from ngt_amd import base, ngtpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_NGT = os.path.join(ROOT, "oracle", "_ref", "ngt")


def same_graph(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2]).view(np.uint32)))


# four batches with incoming edges; a pruned kNN graph in ten batches; a limit
# on the explored edges with a negative epsilon (about a second each)
@pytest.mark.parametrize("name", ["r_b256", "r_k10", "r_E10"])
def test_restatement_reproduces_fixture(name):
    eps, _, k, explore, batch, src = D.CASES[name]
    prop, rows, _, tree = D.index_parts()
    got = R.refine(rows, tree, prop, *D.csr(src), eps, k, None if explore == D.INT_MIN else explore, batch)
    assert same_graph(got, D.csr(name))


def test_fixtures_pin_the_batch_order_and_the_hub():
    assert not same_graph(D.csr("r_b256"), D.csr("r_one"))
    assert not same_graph(D.csr("r_b256"), D.csr("r_a"))
    off = D.csr("r_E10")[0]
    assert int(np.diff(off).max()) == 484
    off = D.csr("r_k30")[0]
    assert set(np.diff(off)[1:].tolist()) == {29, 30}
    assert set(np.diff(D.csr("r_k10")[0])[1:].tolist()) == {10}


def test_restatement_keeps_separated_repeats_and_skips_by_lower_bound():
    # node 1: results bring 2 again at the stored distance (dropped) and 3 at another
    # distance with 4 in between (both stay)
    g = [[], [(2, 1.0), (3, 2.0), (4, 2.5)], [], [], [], []]
    R.merge(g, 1, [[(1, 0.0), (2, 1.0), (3, 3.0)]], False)
    assert g[1] == [(2, 1.0), (3, 2.0), (4, 2.5), (3, 3.0)]
    # addEdge: the position of (1.0, 1) in node 5's list holds id 1 at a larger distance
    g = [[], [], [], [], [], [(1, 1.5), (2, 2.0)]]
    R.merge(g, 1, [[(5, 1.0)]], True)
    assert g[5] == [(1, 1.5), (2, 2.0)] and g[1] == [(5, 1.0)]
    # ... unless an earlier insertion lies between the two
    g = [[], [], [], [], [], [(2, 1.5), (3, 2.0)]]
    R.merge(g, 1, [[(5, 1.2)], [(5, 1.0)]], True)
    assert g[5] == [(2, 1.0), (1, 1.2), (2, 1.5), (3, 2.0)]


@pytest.mark.skipif(not os.path.exists(REF_NGT), reason="the reference CLI (oracle/_ref/ngt) is not built")
def test_recipe_reproduces_committed_fixtures():
    import make_refine_goldens as M
    with tempfile.TemporaryDirectory() as work:
        M.run_recipe(REF_NGT, D.GOLD, work)
        for f in ("grp", "obj", "prf", "tre"):
            assert filecmp.cmp(os.path.join(work, "anng", f), os.path.join(D.REFINE1K, "anng", f), shallow=False), f
        assert filecmp.cmp(os.path.join(work, "anng_t", "prf"), os.path.join(D.REFINE1K, "anng_t", "prf"), shallow=False)
        for name, _, _ in M.OUTPUTS:
            assert filecmp.cmp(os.path.join(work, name, "grp"), os.path.join(D.REFINE1K, name, "grp"), shallow=False), name


# ---- ngt_refine_anng: what is decided before any device work ---------------------
def test_null_index_is_a_parameter_error():
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    assert not L.ngt_refine_anng(None, 0.1, 0.0, 0, D.INT_MIN, 10000, err)
    assert base._err_string(L, err) == "Capi : ngt_refine_anng() : parametor error: index = 0"
    L.ngt_destroy_error_object(err)


def test_argument_errors_leave_the_graph_alone(tmp_path):
    L = ngt_amd.lib()
    src = D.make_index_dir(str(tmp_path / "anng"))
    ix = base.Index(src)
    for args, text in [((0.1, 0.0, 0, D.INT_MIN, 0), "GraphReconstructor::refineANNG: the batch size is 0"),
                       ((0.1, 0.8, 0, D.INT_MIN, 256), "GraphReconstructor::refineANNG: AccuracyTable: The accuracy "
                                                       "table is not set yet. The table size=0"),
                       ((0.1, 0.0, 0, -3, 256), "Invalid edge size parameters -3:0")]:
        assert not L.ngt_refine_anng(ix.index, *args, ix.err)
        msg = base._err_string(L, ix.err)
        assert msg.startswith("Capi : ngt_refine_anng() : Error: ") and text in msg, msg
    out = str(tmp_path / "out")
    ix.save(out)
    ix.close()
    for f in ("grp", "prf", "obj", "tre"):
        assert filecmp.cmp(os.path.join(out, f), os.path.join(src, f), shallow=False), f


def test_accuracy_table_of_two_entries_is_not_set():
    # AccuracyTable::getEpsilon refuses a table of two entries or fewer (Index.h:318); the r_a
    # fixture pins the interpolation itself on the device
    L = ngt_amd.lib()
    with tempfile.TemporaryDirectory() as t:
        src = D.make_index_dir(os.path.join(t, "anng"))
        lines = [l for l in open(os.path.join(src, "prf")) if not l.startswith("AccuracyTable\t")]
        with open(os.path.join(src, "prf"), "w") as f:
            f.writelines(sorted(lines + ["AccuracyTable\t-0.5:0.2,0.1:0.9\n"]))
        ix = base.Index(src)
        assert not L.ngt_refine_anng(ix.index, 0.1, 0.8, 0, D.INT_MIN, 256, ix.err)
        assert "The table size=2" in base._err_string(L, ix.err)
        ix.close()


# ---- C++ and Python surfaces ---------------------------------------------------------
def test_header_and_sample_compile_without_warnings(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "refine_sample"), os.path.join(ROOT, "tests", "cxx", "refine_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
    # both overloads of the reference resolve (GraphReconstructor.h:803, :814)
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "NGT/GraphReconstructor.h"\n'
                     "void f(NGT::Index& i) {\n"
                     "  NGT::GraphReconstructor::refineANNG(i);\n"
                     "  NGT::GraphReconstructor::refineANNG(i, true);\n"
                     "  NGT::GraphReconstructor::refineANNG(i, 0.1f, 0.0f, 0, INT_MIN, (size_t)10000);\n"
                     "  NGT::GraphReconstructor::refineANNG(i, false, 0.1f, 0.0f, 0, INT_MIN, (size_t)10000);\n"
                     "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", "-o", str(tmp_path / "probe.o"), str(probe)])


def test_ngtpy_refine_anng_has_the_reference_signature():
    sig = inspect.signature(ngtpy.Index.refine_anng)
    got = [(p.name, p.default) for p in list(sig.parameters.values())[1:]]
    assert got == [("epsilon", 0.1), ("expected_accuracy", 0.0), ("num_of_edges", 0),
                   ("num_of_explored_edges", -2 ** 31), ("batch_size", 10000)]
