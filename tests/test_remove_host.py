"""CPU-side checks of object removal: the plain-Python restatement
(tests/remove_restate.py) against the reference-built fixtures
(tests/golden/remove1k), the fixture recipe, the two lower_bound rules, the
argument check of `ngt_remove_index` that needs no device and the C++ header
(no device call is made here)."""
import filecmp
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ngt_amd
import remove_data as D
import remove_restate as R
from ngt_amd import base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_NGT = os.path.join(ROOT, "oracle", "_ref", "ngt")


def restated(case):
    e = D.expected()[case]
    rows, valid, offs, ids, dists, tree, prop = D.load_input(e["input"])
    ix = R.Index("l2", rows, valid, offs, ids, dists, tree, D.leaf_lists(tree), int(prop["EdgeSizeForSearch"]))
    done = [int(ix.remove(i)) for i in e["ids"]]
    return e, ix, done


# the hub and the lists it edited, three refusals; tree replace both ways; a
# directed graph with missing reverse edges; a root leaf emptied to the last node
@pytest.mark.parametrize("case", ["rm_seq", "rm_dup", "rm_onng", "rm_all"])
def test_restatement_reproduces_fixture(case):
    e, ix, done = restated(case)
    assert done == e["removed"]
    offs, ids, dists = ix.csr()
    want = D.F.read_grp(os.path.join(D.RM, case, "grp"))
    assert np.array_equal(offs, want[0]) and np.array_equal(ids, want[1])
    assert np.array_equal(dists.view(np.uint32), want[2].view(np.uint32))
    if case == "rm_all":
        # the reference writes the emptied root leaf with its pivot, which no
        # reader of the format takes back (Node.h:466-512): compare the counts
        raw = open(os.path.join(D.RM, case, "tre"), "rb").read()
        assert raw[:8] == (2).to_bytes(8, "little") and raw[8:9] == b"-" and raw[9:10] == b"+"
        assert int.from_bytes(raw[18:20], "little") == 0 and ix.leaves[1] == []
        return
    tree = D.F.read_tre(os.path.join(D.RM, case, "tre"), 128, np.float32)
    assert ix.leaves == D.leaf_lists(tree)


def test_fixtures_pin_the_hub_the_refusals_and_the_emptied_leaf():
    e = D.expected()
    _, _, offs, ids, _, tree, _ = D.load_input("anng")
    assert int(offs[18] - offs[17]) == 439 and e["rm_seq"]["ids"][0] == 17
    assert e["rm_seq"]["ids"][1:21] == [int(v) for v in ids[int(offs[17]):int(offs[17]) + 20]]
    assert e["rm_seq"]["removed"] == [1] * 21 + [0, 0, 0]
    assert 0 in e["rm_onng"]["removed"]
    assert e["rm_oneleaf"]["ids"] == sorted(D.leaf_lists(tree)[22]) and len(e["rm_oneleaf"]["ids"]) == 47
    after = D.F.read_tre(os.path.join(D.RM, "rm_oneleaf", "tre"), 128, np.float32)
    assert D.leaf_lists(after)[22] == [] and after["leaf_valid"][22] == 1
    rows = D.load_input("dup")[0]
    assert np.array_equal(rows[901:1001], rows[1:101])


def test_reverse_edge_at_another_distance_is_not_erased():
    lst = [(1.0, 4), (2.0, 7), (3.0, 9)]
    assert not R.erase_reverse_edge(lst, 2.5, 7) and lst == [(1.0, 4), (2.0, 7), (3.0, 9)]
    assert not R.erase_reverse_edge(lst, 0.5, 7) and len(lst) == 3  # lands on (1.0, 4)
    assert R.erase_reverse_edge(lst, 2.0, 7) and lst == [(1.0, 4), (3.0, 9)]
    # a smaller stored distance finds the edge when nothing lies in between: one position is looked at
    lst = [(1.0, 4), (2.0, 7), (3.0, 9)]
    assert R.erase_reverse_edge(lst, 1.5, 7) and lst == [(1.0, 4), (3.0, 9)]


def test_id_at_the_insert_position_is_not_inserted_twice():
    lst = [(1.0, 4), (2.0, 7), (3.0, 9)]
    assert not R.insert_edge(lst, 1.5, 7) and lst == [(1.0, 4), (2.0, 7), (3.0, 9)]
    # ... but an id further down the list is: the rule looks at one position only
    assert R.insert_edge(lst, 0.5, 7) and lst == [(0.5, 7), (1.0, 4), (2.0, 7), (3.0, 9)]


def test_relink_chain_takes_the_first_minimum_of_the_current_order():
    rows = np.zeros((6, 16), np.float32)
    rows[1:, 0] = [0.0, 3.0, 1.0, 1.0, 3.0]
    rows.setflags(write=False)
    # from 1 the nearest are 3 and 4 (tie: the earlier position, 3); 3 moves next to 1 and 2 to its place
    links = R.relink_chain("l2", rows, [1, 2, 3, 4, 5])
    assert [(a, b) for a, b, _ in links] == [(1, 3), (3, 4), (4, 2), (2, 5)]
    assert [float(d) for _, _, d in links] == [1.0, 0.0, 2.0, 0.0]


@pytest.mark.skipif(not os.path.exists(REF_NGT), reason="the reference CLI (oracle/_ref/ngt) is not built")
def test_recipe_reproduces_committed_fixtures():
    import make_remove_goldens as M
    with tempfile.TemporaryDirectory() as work:
        records = M.run_recipe(REF_NGT, D.GOLD, work)
        assert records == D.expected()
        for name, files in (("dup", ("grp", "obj", "prf", "tre")), ("tiny", ("grp", "obj", "prf", "tre")),
                            ("onng", ("grp", "prf"))):
            for f in files:
                assert filecmp.cmp(os.path.join(work, name, f), os.path.join(D.RM, name, f), shallow=False), (name, f)
        for name, _ in M.CASES:
            for f in ("grp", "tre"):
                assert filecmp.cmp(os.path.join(work, name, f), os.path.join(D.RM, name, f), shallow=False), (name, f)


def test_null_index_is_a_parameter_error():
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    assert not L.ngt_remove_index(None, 1, err)
    assert base._err_string(L, err) == "Capi : ngt_remove_index() : parametor error: index = 0"
    assert not L.ngt_batch_remove_index(None, None, 0, None, err)
    assert base._err_string(L, err) == "Capi : ngt_batch_remove_index() : parametor error: index = 0"
    L.ngt_destroy_error_object(err)


def test_header_and_sample_compile_without_warnings(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "remove_sample"), os.path.join(ROOT, "tests", "cxx", "remove_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
