"""CPU-side checks of the ONNG reconstruction: the plain-Python restatement
(tests/onng_restate.py) against the reference-built fixtures, the fixture
recipe, and the host logic of the `ngt_optimizer_*` C API and ngtpy.Optimizer
(no device call is made here)."""
import ctypes
import filecmp
import os
import tempfile

import numpy as np
import pytest

import ngt_amd
import onng_data as D
import onng_restate as R
from ngt_amd import base, ngtpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_NGT = os.path.join(ROOT, "oracle", "_ref", "ngt")

DEFAULTS = dict(num_of_outgoings=10, num_of_incomings=120, min_num_of_edges=0, num_of_queries=100,
                num_of_objects=20, low_accuracy_from=np.float32(0.30), low_accuracy_to=np.float32(0.50),
                high_accuracy_from=np.float32(0.80), high_accuracy_to=np.float32(0.90), gt_epsilon=0.1, margin=0.2,
                log_disabled=0, shortcut_reduction=1, search_parameter_optimization=1,
                prefetch_parameter_optimization=1, accuracy_table_generation=1)


def same_graph(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2]).view(np.uint32)))


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_restatement_reproduces_fixture(name):
    o, i, path, min_edges, src = D.CASES[name]
    off, ids, d = D.csr(src)
    got = R.reconstruct(off, ids, d, o, i, path, min_edges, input_is_anng=(src == "anng"))
    assert same_graph(got, D.csr(name))


def test_fixture_takes_the_short_node_branch():
    # onng_R: -o 30 on the converted onng_S; nodes with fewer than 30 entries keep their stored list
    off, ids, d = D.csr("onng_S")
    conv = R.convert_to_anng(R.from_csr(off, ids, d))
    assert sum(1 for v in range(1, len(conv)) if len(conv[v]) < 30) == 1379


@pytest.mark.skipif(not os.path.exists(REF_NGT), reason="the reference CLI (oracle/_ref/ngt) is not built")
def test_recipe_reproduces_committed_fixtures():
    import make_onng_goldens as M
    with tempfile.TemporaryDirectory() as work:
        M.run_recipe(REF_NGT, os.path.join(D.GOLD, "sift5k.npy"), work)
        assert open(os.path.join(work, "anng", "grp"), "rb").read() == D.anng_grp_bytes()
        for name, _, _ in M.OUTPUTS:
            assert filecmp.cmp(os.path.join(work, name, "grp"), os.path.join(D.ONNG2K, name, "grp"), shallow=False), name


# ---- ngt_optimizer_* -----------------------------------------------------------
class Opt(object):
    def __init__(self):
        self.L = ngt_amd.lib()
        self.err = self.L.ngt_create_error_object()
        self.opt = self.L.ngt_create_optimizer(False, self.err)
        assert self.opt

    def get(self):
        v = (ctypes.c_double * 16)()
        assert self.L.ngt_optimizer_get(self.opt, v, self.err)
        return dict(zip(DEFAULTS, list(v)))

    def error(self):
        return base._err_string(self.L, self.err)

    def close(self):
        self.L.ngt_destroy_optimizer(self.opt)
        self.L.ngt_destroy_error_object(self.err)


@pytest.fixture
def opt():
    o = Opt()
    yield o
    o.close()


def test_optimizer_defaults(opt):
    assert opt.get() == {k: float(v) for k, v in DEFAULTS.items()}


def test_optimizer_negative_or_zero_keeps_the_value(opt):
    L = opt.L
    assert L.ngt_optimizer_set_minimum(opt.opt, -1, -1, 0, 0, opt.err)
    assert L.ngt_optimizer_set_extension(opt.opt, 0.0, -1.0, 0.0, -1.0, -1.5, 0.0, opt.err)
    assert L.ngt_optimizer_set(opt.opt, -1, -1, -1, -1.0, -1.0, -1.0, -1.0, -2.0, -1.0, opt.err)
    assert opt.get() == {k: float(v) for k, v in DEFAULTS.items()}
    # zero is a value for the edge counts, and gt epsilon takes anything from -1 up
    assert L.ngt_optimizer_set_minimum(opt.opt, 0, 0, 7, 9, opt.err)
    assert L.ngt_optimizer_set_extension(opt.opt, 0.1, 0.2, 0.3, 0.4, -1.0, 0.5, opt.err)
    g = opt.get()
    assert (g["num_of_outgoings"], g["num_of_incomings"], g["num_of_queries"], g["num_of_objects"]) == (0, 0, 7, 9)
    assert g["low_accuracy_from"] == np.float32(0.1) and g["high_accuracy_to"] == np.float32(0.4)
    assert g["gt_epsilon"] == -1.0 and g["margin"] == 0.5
    # the obsolete nine-argument set leaves the number of results alone
    assert L.ngt_optimizer_set(opt.opt, 5, 40, 11, -1.0, -1.0, -1.0, -1.0, 0.25, -1.0, opt.err)
    g = opt.get()
    assert (g["num_of_outgoings"], g["num_of_incomings"], g["num_of_queries"], g["num_of_objects"]) == (5, 40, 11, 9)
    assert g["gt_epsilon"] == 0.25 and g["margin"] == 0.5


def test_optimizer_processing_modes(opt):
    L = opt.L
    assert L.ngt_optimizer_set_processing_modes(opt.opt, False, True, False, opt.err)
    g = opt.get()
    assert (g["shortcut_reduction"], g["search_parameter_optimization"], g["prefetch_parameter_optimization"],
            g["accuracy_table_generation"]) == (1, 0, 1, 0)
    assert L.ngt_optimizer_set_shortcut_reduction(opt.opt, False, 12, opt.err)
    g = opt.get()
    assert g["shortcut_reduction"] == 0 and g["min_num_of_edges"] == 12


def test_null_optimizer_error_strings():
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    calls = {
        "ngt_optimizer_adjust_search_coefficients": lambda: L.ngt_optimizer_adjust_search_coefficients(None, b"x", err),
        "ngt_optimizer_execute": lambda: L.ngt_optimizer_execute(None, b"a", b"b", err),
        "ngt_optimizer_set": lambda: L.ngt_optimizer_set(None, 1, 1, 1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, err),
        "ngt_optimizer_set_minimum": lambda: L.ngt_optimizer_set_minimum(None, 1, 1, 1, 1, err),
        "ngt_optimizer_set_extension": lambda: L.ngt_optimizer_set_extension(None, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, err),
        "ngt_optimizer_set_processing_modes": lambda: L.ngt_optimizer_set_processing_modes(None, False, False, False,
                                                                                         err),
    }
    for name, call in calls.items():
        L.ngt_clear_error_string(err)
        assert not call()
        # Capi.cpp:872-876: "parametor error: optimizer = " << optimizer, a null pointer streams as 0
        assert base._err_string(L, err) == "Capi : %s() : parametor error: optimizer = 0" % name
    L.ngt_destroy_optimizer(None)
    L.ngt_destroy_error_object(err)


def test_execute_refuses_while_a_tuning_mode_is_on(opt, tmp_path):
    src = D.make_anng_dir(str(tmp_path / "anng"))
    out = str(tmp_path / "out")
    for modes in [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]:
        assert opt.L.ngt_optimizer_set_processing_modes(opt.opt, *modes, opt.err)
        assert not opt.L.ngt_optimizer_execute(opt.opt, src.encode(), out.encode(), opt.err)
        assert "ngt_optimizer_set_processing_modes(opt, false, false, false) is required" in opt.error()
        assert not os.path.exists(out)


def test_execute_refuses_an_existing_output_path(opt, tmp_path):
    src = D.make_anng_dir(str(tmp_path / "anng"))
    out = tmp_path / "out"
    out.mkdir()
    assert opt.L.ngt_optimizer_set_processing_modes(opt.opt, False, False, False, opt.err)
    assert not opt.L.ngt_optimizer_execute(opt.opt, src.encode(), str(out).encode(), opt.err)
    assert opt.error() == ("Capi : ngt_optimizer_execute() : Error: Optimizer::execute: "
                           "The specified index exists. %s" % out)
    assert os.listdir(str(out)) == []


def test_execute_reports_a_missing_input(opt, tmp_path):
    out = str(tmp_path / "out")
    assert opt.L.ngt_optimizer_set_processing_modes(opt.opt, False, False, False, opt.err)
    assert not opt.L.ngt_optimizer_execute(opt.opt, str(tmp_path / "nothing").encode(), out.encode(), opt.err)
    assert "Optimizer::execute: Cannot create the specified index. " + out in opt.error()
    assert not os.path.exists(out)


# ---- ngtpy.Optimizer ---------------------------------------------------------
def test_ngtpy_optimizer_maps_its_arguments():
    assert ngtpy.Optimizer().get() == {k: float(v) for k, v in DEFAULTS.items()}
    o = ngtpy.Optimizer(num_of_outgoings=5, num_of_incomings=40, num_of_queries=33, num_of_objects=44,
                        low_accuracy_from=0.11, low_accuracy_to=0.22, high_accuracy_from=0.66, high_accuracy_to=0.77,
                        gt_epsilon=0.05, margin=0.3, log_disabled=True)
    g = o.get()
    want = dict(DEFAULTS, num_of_outgoings=5, num_of_incomings=40, num_of_queries=33, num_of_objects=44,
                low_accuracy_from=np.float32(0.11), low_accuracy_to=np.float32(0.22),
                high_accuracy_from=np.float32(0.66), high_accuracy_to=np.float32(0.77), gt_epsilon=0.05, margin=0.3,
                log_disabled=1)
    assert g == {k: float(v) for k, v in want.items()}
    o.set(num_of_incomings=0)
    assert o.get()["num_of_incomings"] == 0 and o.get()["num_of_outgoings"] == 5
    o.set_processing_modes(False, False, True, False)
    g = o.get()
    assert (g["shortcut_reduction"], g["search_parameter_optimization"], g["prefetch_parameter_optimization"],
            g["accuracy_table_generation"]) == (0, 0, 1, 0)
    o.set_processing_modes(search_parameter_optimization=False)
    g = o.get()
    assert (g["shortcut_reduction"], g["search_parameter_optimization"], g["prefetch_parameter_optimization"],
            g["accuracy_table_generation"]) == (1, 0, 1, 1)


def test_ngtpy_optimizer_execute_raises_the_c_api_error(tmp_path):
    src = D.make_anng_dir(str(tmp_path / "anng"))
    with pytest.raises(ngt_amd.NativeError, match="set_processing_modes"):
        ngtpy.Optimizer().execute(src, str(tmp_path / "out"))
    assert not os.path.exists(str(tmp_path / "out"))
