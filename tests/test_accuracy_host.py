"""CPU-side checks of the accuracy-table generation: the plain-Python
restatement (tests/accuracy_restate.py) over the CPU oracle against the
reference's tables (tests/golden/accuracy_tables.json), the pure host unit
(ngt_amd/csrc/accuracy_table.cpp) through tests/cxx/accuracy_table_host.cpp,
and the refusals of the C API, the C++ facade and ngtpy that are decided
before any device call."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import accuracy_restate as A
import ngt_amd
import ngt_files as F
import onng_restate as OR
from ngt_amd import base, ngtpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_NGT = os.path.join(ROOT, "oracle", "_ref", "ngt")
TABLES = json.load(open(os.path.join(GOLD, "accuracy_tables.json")))
# case -> (number of results, number of queries): the -n and -q of its command
CASES = {"c1_onng": (20, 100), "refine1k": (20, 100), "refine1k_q40": (30, 40), "refine1k_onng": (20, 100),
         "acctab_f16": (20, 100), "acctab_u24": (20, 100)}
# maxEpsilon of the reference's own loop, 6 digits (read once from a probe built on the reference's headers)
MAX_EPSILON = {"c1_onng": "0.378598", "refine1k": "0.238598", "refine1k_onng": "0.342318", "acctab_f16": "0.302318",
               "acctab_u24": "0.258598"}
EDGE_REFUSAL = ("Optimizer::generateAccuracyTable: edgeSizeForSearch is invalid to call generateAccuracyTable, "
                "because accuracy 1.0 cannot be achieved with the setting. edgeSizeForSearch=40.")


def load_case(name):
    d = os.path.join(GOLD, TABLES[name]["source"])
    prop = F.read_prf(os.path.join(d, "prf"))
    dim = int(prop["Dimension"])
    dt = np.uint8 if prop["ObjectType"].startswith("Integer") else np.float32
    rows, valid = F.read_obj(os.path.join(d, "obj"), dim, dt)
    offs, ids, dists = F.read_grp(os.path.join(d, "grp"))
    tree = F.read_tre(os.path.join(d, "tre"), dim, dt)
    if name == "refine1k_onng":  # reconstruct-graph -m S -o 10 -i 120 comes first
        offs, ids, dists = OR.reconstruct(offs, ids, dists, 10, 120, True, 0, input_is_anng=True)
    return prop, rows, valid, offs, ids, tree


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference_table(name):
    prop, rows, valid, offs, ids, tree = load_case(name)
    search = A.oracle_search(rows, tree, prop, offs, ids)
    nresults, nqueries = CASES[name]
    pairs, text, maxeps = A.generate(search, rows, valid, prop, nresults, nqueries)
    assert text == TABLES[name]["table"]
    if name in MAX_EPSILON:
        assert A.fmt(maxeps) == MAX_EPSILON[name]
    # the work guard at 40 x changes nothing: the identity rule alone gives the same
    _, text2, maxeps2 = A.generate(search, rows, valid, prop, nresults, nqueries, guard=None)
    assert (text2, maxeps2) == (text, maxeps)


def test_reference_prf_differs_from_its_source_in_the_table_alone():
    for name in CASES:
        src = open(os.path.join(GOLD, TABLES[name]["source"], "prf")).read().split("\n")
        got = TABLES[name]["prf"].split("\n")
        diff = {a.split("\t")[0] for a, b in zip(src, got) if a != b}
        assert len(src) == len(got)
        assert diff <= ({"AccuracyTable", "GraphType"} if name == "refine1k_onng" else {"AccuracyTable"}), name
    assert TABLES["c1_onng"]["prf"] == open(os.path.join(GOLD, "c1_onng", "prf")).read()


def test_restatement_refusals():
    prop = F.read_prf(os.path.join(GOLD, "c1_anng", "prf"))
    assert TABLES["c1_anng"]["error"].endswith(A.refusal(prop, 20))
    prop = F.read_prf(os.path.join(GOLD, "refine1k", "anng", "prf"))
    assert TABLES["refine1k_n10"]["error"].endswith(A.refusal(prop, 10))
    assert A.refusal(prop, 20) is None


@pytest.mark.skipif(not os.path.exists(REF_NGT), reason="the reference CLI (oracle/_ref/ngt) is not built")
def test_recipe_reproduces_its_clock_free_parts(tmp_path):
    """The parts of the fixture recipe no clock enters: `ngt create` of the two
    small indexes, and the reference's two refusals.  The reference's table
    generation itself is not re-run here: it holds a wall-clock clause
    (Optimizer.h:1461), so a loaded machine can change its result; the recipe
    guards against that when a person regenerates the fixtures."""
    import make_accuracy_table_goldens as M
    M.create_small_indexes(REF_NGT, str(tmp_path))
    for name in M.CREATE:
        for f in ("grp", "obj", "prf", "tre"):
            assert open(str(tmp_path / name / f), "rb").read() == open(os.path.join(GOLD, name, f), "rb").read(), \
                (name, f)
    for name, src, command, args in M.CASES:
        if "error" in TABLES[name]:
            # c1_anng is refused before any search; refine1k_n10's ground truth is too short at any maxEpsilon
            assert M.run_case(REF_NGT, os.path.join(GOLD, src), command, args, str(tmp_path)) == \
                ("error", TABLES[name]["error"]), name


# ---- the pure host unit, without Python in the loop -----------------------------
def build_host_program(exe, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "accuracy_table_host.cpp"),
                           os.path.join(ROOT, "ngt_amd", "csrc", "accuracy_table.cpp")])


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_host_unit_reproduces_the_recorded_run(tmp_path, flags):
    exe = str(tmp_path / "accuracy_table_host")
    build_host_program(exe, flags)
    r = subprocess.run([exe, os.path.join(GOLD, "accuracy_trace_c1_onng.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: ") and "maxEpsilon 0.378598" in r.stdout


# ---- refusals that need no device ----------------------------------------------
class Opt(object):
    def __init__(self, modes=None, queries=0, results=0):
        self.L = ngt_amd.lib()
        self.err = self.L.ngt_create_error_object()
        self.opt = self.L.ngt_create_optimizer(True, self.err)
        assert self.opt
        if modes is not None:
            assert self.L.ngt_optimizer_set_processing_modes(self.opt, *modes, self.err)
        assert self.L.ngt_optimizer_set_minimum(self.opt, 0, 0, queries, results, self.err)

    def run(self, path):
        self.L.ngt_clear_error_string(self.err)
        ok = self.L.ngt_optimizer_optimize_search_parameters(self.opt, os.fsencode(path), self.err)
        return ok, base._err_string(self.L, self.err)

    def close(self):
        self.L.ngt_destroy_optimizer(self.opt)
        self.L.ngt_destroy_error_object(self.err)


def snapshot(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_null_arguments():
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    assert not L.ngt_optimizer_optimize_search_parameters(None, b"x", err)
    assert base._err_string(L, err) == \
        "Capi : ngt_optimizer_optimize_search_parameters() : parametor error: optimizer = 0"
    o = Opt()
    assert not L.ngt_optimizer_optimize_search_parameters(o.opt, None, err)
    assert base._err_string(L, err) == \
        "Capi : ngt_optimizer_optimize_search_parameters() : parametor error: index path = 0"
    o.close()
    assert not L.ngt_generate_accuracy_table(None, 20, 100, err)
    assert base._err_string(L, err) == "Capi : ngt_generate_accuracy_table() : parametor error: index = 0"
    L.ngt_destroy_error_object(err)


def test_refuses_while_a_timing_driven_mode_is_on(tmp_path):
    idx = str(tmp_path / "anng")
    shutil.copytree(os.path.join(GOLD, "refine1k", "anng"), idx)
    before = snapshot(idx)
    for modes in [None, (True, False, True), (False, True, True), (True, True, False)]:
        o = Opt(modes)
        ok, msg = o.run(idx)
        o.close()
        assert not ok
        assert "ngt_optimizer_set_processing_modes(opt, false, false, true)" in msg
        assert snapshot(idx) == before


def test_all_modes_off_writes_nothing(tmp_path):
    idx = str(tmp_path / "anng")
    shutil.copytree(os.path.join(GOLD, "refine1k", "anng"), idx)
    before = snapshot(idx)
    o = Opt((False, False, False))
    assert o.run(idx) == (True, "")
    # the reference opens nothing in that case: not even a missing path is noticed
    assert o.run(str(tmp_path / "nothing")) == (True, "")
    o.close()
    assert snapshot(idx) == before


def test_refuses_an_edge_size_that_cannot_reach_accuracy_one(tmp_path):
    idx = str(tmp_path / "c1_anng")
    shutil.copytree(os.path.join(GOLD, "c1_anng"), idx)
    before = snapshot(idx)
    o = Opt((False, False, True))
    ok, msg = o.run(idx)
    o.close()
    assert not ok
    assert msg == "Capi : ngt_optimizer_optimize_search_parameters() : Error: " + TABLES["c1_anng"]["error"]
    assert TABLES["c1_anng"]["error"].endswith(EDGE_REFUSAL)
    assert snapshot(idx) == before
    # the same on a live handle
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    index = L.ngt_open_index(idx.encode(), err)
    assert index
    assert not L.ngt_generate_accuracy_table(index, 20, 100, err)
    assert base._err_string(L, err) == "Capi : ngt_generate_accuracy_table() : Error: " + EDGE_REFUSAL
    L.ngt_close_index(index)
    L.ngt_destroy_error_object(err)


def test_refuses_fewer_results_than_the_sweep_searches(tmp_path):
    idx = str(tmp_path / "anng")
    shutil.copytree(os.path.join(GOLD, "refine1k", "anng"), idx)
    before = snapshot(idx)
    o = Opt((False, False, True), queries=50, results=10)
    ok, msg = o.run(idx)
    o.close()
    assert not ok
    assert msg == "Capi : ngt_optimizer_optimize_search_parameters() : Error: " + TABLES["refine1k_n10"]["error"]
    assert snapshot(idx) == before


def test_reports_a_missing_index(tmp_path):
    o = Opt((False, False, True))
    ok, msg = o.run(str(tmp_path / "nothing"))
    o.close()
    assert not ok and "Optimizer::execute: Cannot generate the accuracy table. " in msg


def test_ngtpy_optimizer_raises_the_c_api_error(tmp_path):
    idx = str(tmp_path / "c1_anng")
    shutil.copytree(os.path.join(GOLD, "c1_anng"), idx)
    o = ngtpy.Optimizer(log_disabled=True)
    with pytest.raises(ngt_amd.NativeError, match="false, false, true"):
        o.optimize_search_parameters(idx)
    o.set_processing_modes(search_parameter_optimization=False, prefetch_parameter_optimization=False)
    with pytest.raises(ngt_amd.NativeError, match="edgeSizeForSearch=40"):
        o.optimize_search_parameters(idx)


def test_cxx_facade_reports_the_refusals(tmp_path):
    exe = str(tmp_path / "accuracy_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "accuracy_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
    idx = str(tmp_path / "c1_anng")
    shutil.copytree(os.path.join(GOLD, "c1_anng"), idx)
    r = subprocess.run([exe, idx], capture_output=True, text=True)
    assert r.returncode == 1 and EDGE_REFUSAL in r.stderr
    r = subprocess.run([exe, idx, "100", "20", "s"], capture_output=True, text=True)
    assert r.returncode == 1 and "false, false, true" in r.stderr
