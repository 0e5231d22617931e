"""Accuracy-table generation on the device: ngt_optimizer_optimize_search_parameters,
ngt_generate_accuracy_table, ngt_amd_accuracy_table, ngtpy and
NGT/GraphOptimizer.h against the prf files the reference wrote
(tests/golden/accuracy_tables.json, make_accuracy_table_goldens.py).  Every
comparison is exact: the prf byte for byte."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ngt_amd
import ngt_files as F
from ngt_amd import base, ngtpy
from ngt_amd.device import DeviceIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TABLES = json.load(open(os.path.join(GOLD, "accuracy_tables.json")))
CASES = {"c1_onng": (20, 100), "refine1k": (20, 100), "refine1k_q40": (30, 40), "refine1k_onng": (20, 100),
         "acctab_f16": (20, 100), "acctab_u24": (20, 100)}


class Opt(object):
    def __init__(self, modes, queries=0, results=0, outgoing=-1, incoming=-1):
        self.L = ngt_amd.lib()
        self.err = self.L.ngt_create_error_object()
        self.opt = self.L.ngt_create_optimizer(True, self.err)
        assert self.opt
        assert self.L.ngt_optimizer_set_processing_modes(self.opt, *modes, self.err)
        assert self.L.ngt_optimizer_set_minimum(self.opt, outgoing, incoming, queries, results, self.err)

    def check(self, ok):
        assert ok, base._err_string(self.L, self.err)

    def close(self):
        self.L.ngt_destroy_optimizer(self.opt)
        self.L.ngt_destroy_error_object(self.err)


def blank_copy(name, dst):
    """A copy of the case's source index with an empty AccuracyTable."""
    shutil.copytree(os.path.join(GOLD, TABLES[name]["source"]), dst)
    prf = os.path.join(dst, "prf")
    lines = [("AccuracyTable\t\n" if l.split("\t")[0] == "AccuracyTable" else l) for l in open(prf)]
    with open(prf, "w") as f:
        f.writelines(lines)
    return dst


def read(d, f):
    return open(os.path.join(d, f), "rb").read()


def generate(name, idx):
    nresults, nqueries = CASES[name]
    o = Opt((False, False, True), nqueries, nresults)
    o.check(o.L.ngt_optimizer_optimize_search_parameters(o.opt, idx.encode(), o.err))
    o.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_optimize_search_parameters_writes_the_reference_prf(name, tmp_path):
    idx = blank_copy(name, str(tmp_path / "in"))
    if name == "refine1k_onng":
        # end to end: the graph stages of `reconstruct-graph -m S -o 10 -i 120`, then its `-s a` tail
        o = Opt((False, False, False), outgoing=10, incoming=120)
        out = str(tmp_path / "out")
        o.check(o.L.ngt_optimizer_execute(o.opt, idx.encode(), out.encode(), o.err))
        o.close()
        idx = out
    before = {f: read(idx, f) for f in ("grp", "obj", "tre")}
    generate(name, idx)
    assert read(idx, "prf").decode() == TABLES[name]["prf"]
    assert {f: read(idx, f) for f in ("grp", "obj", "tre")} == before
    assert sorted(os.listdir(idx)) == ["grp", "obj", "prf", "tre"]


@pytest.mark.parametrize("knob", ["NGT_AMD_LA", "NGT_AMD_LAT"])
def test_table_does_not_depend_on_the_search_kernel(knob, tmp_path, monkeypatch):
    monkeypatch.setenv(knob, "0")
    idx = blank_copy("refine1k", str(tmp_path / "in"))
    generate("refine1k", idx)
    assert read(idx, "prf").decode() == TABLES["refine1k"]["prf"]


def test_generate_on_a_handle_then_save_and_search(tmp_path):
    idx = blank_copy("acctab_f16", str(tmp_path / "in"))
    ix = ngtpy.Index(idx)
    q = np.random.RandomState(3).rand(16).astype(np.float32)
    with pytest.raises(ngt_amd.NativeError, match="The accuracy table is not set yet"):
        ix.search(q, expected_accuracy=0.9)
    table = ix.generate_accuracy_table()
    want = [(float(np.float32(float(e))), float(a)) for e, a in
            (t.split(":") for t in TABLES["acctab_f16"]["table"].split(","))]
    assert table == want
    # a search with an expected accuracy works at once and is the search at the table's epsilon
    eps = ix.epsilon_for(0.9)
    lo = max(e for e, a in table if a < 0.9)
    hi = min(e for e, a in table if a >= 0.9)
    assert lo <= eps <= hi
    assert ix.search(q, size=10, expected_accuracy=0.9) == ix.search(q, size=10, epsilon=eps)
    # refine-anng reads the handle's table too
    ix.refine_anng(expected_accuracy=0.9, batch_size=256)
    # ... and the table is still the handle's afterwards (the prf on disk has none)
    assert ix.epsilon_for(0.9) == eps
    assert len(ix.search(q, size=10, expected_accuracy=0.9)) == 10
    ix.close()
    # ngt_save_index writes the table: the prf of the reference
    ix = ngtpy.Index(idx)
    ix.generate_accuracy_table()
    ix.save()
    ix.close()
    assert read(idx, "prf").decode() == TABLES["acctab_f16"]["prf"]
    for f in ("grp", "obj", "tre"):
        assert read(idx, f) == read(os.path.join(GOLD, "acctab_f16"), f), f


def test_device_api_returns_the_pairs_and_max_epsilon():
    d = os.path.join(GOLD, "acctab_u24")
    prop = F.read_prf(os.path.join(d, "prf"))
    rows, valid = F.read_obj(os.path.join(d, "obj"), 24, np.uint8)
    offs, ids, _ = F.read_grp(os.path.join(d, "grp"))
    ix = DeviceIndex("l2", "uint8", 24, device=0)
    ix.set_objects(rows, valid)
    ix.set_graph(offs, ids)
    ix.set_search_property(40, int(prop["DynamicEdgeSizeBase"]), int(prop["DynamicEdgeSizeRate"]),
                           int(prop["SeedSize"]), 0)
    with pytest.raises(ngt_amd.NativeError, match="edgeSizeForSearch=40"):
        ix.accuracy_table()
    ix.set_search_property(int(prop["EdgeSizeForSearch"]), int(prop["DynamicEdgeSizeBase"]),
                           int(prop["DynamicEdgeSizeRate"]), int(prop["SeedSize"]), 0)
    with pytest.raises(ngt_amd.NativeError, match="needs a graph and a tree"):
        ix.accuracy_table()
    ix.set_tree(F.read_tre(os.path.join(d, "tre"), 24, np.uint8))
    with pytest.raises(ngt_amd.NativeError, match="gt data is less than result size! 19:20"):
        ix.accuracy_table(num_of_results=19)
    # refused before anything of that size is allocated
    with pytest.raises(ngt_amd.NativeError, match="results asked of a repository of 1001 slots"):
        ix.accuracy_table(num_of_results=2 ** 40)
    with pytest.raises(ngt_amd.NativeError, match="queries asked of a repository of 1001 slots"):
        ix.accuracy_table(num_of_queries=2 ** 40)
    pairs, maxeps = ix.accuracy_table()
    ix.close()
    assert ",".join("%g:%g" % (e, a) for e, a in pairs) == TABLES["acctab_u24"]["table"]
    assert "%g" % maxeps == "0.258598"


def test_cxx_facade_and_ngtpy_optimizer(tmp_path):
    exe = str(tmp_path / "accuracy_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "accuracy_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
    idx = blank_copy("refine1k_q40", str(tmp_path / "cxx"))
    r = subprocess.run([exe, idx, "40", "30"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert read(idx, "prf").decode() == TABLES["refine1k_q40"]["prf"]
    idx = blank_copy("acctab_u24", str(tmp_path / "py"))
    o = ngtpy.Optimizer(log_disabled=True)
    o.set_processing_modes(search_parameter_optimization=False, prefetch_parameter_optimization=False)
    o.optimize_search_parameters(idx)
    assert read(idx, "prf").decode() == TABLES["acctab_u24"]["prf"]
