"""Edge-count optimisation on the device: ngt_amd_recut_anng against the numpy
restatement of the re-cut (tests/edges_data.py), and ngt_optimize_number_of_edges,
its returning form, ngtpy and NGT/GraphOptimizer.h against what the reference's
`ngt optimize-#-of-edges` printed and wrote (tests/golden/edge_optimization.json,
make_edge_optimization_goldens.py).  Every comparison is exact: ids and
distance bits of the re-cut graphs, the prf byte for byte."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import edges_data as D
import ngt_amd
import ngt_files as F
from ngt_amd import _sigs, base, edges, ngtpy, onng

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLD, "edge_optimization.json")))
KS = (1, 5, 10, 64, 65)


# ---- the re-cut kernel -----------------------------------------------------------
def csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    ids, ds = [], []
    for v, l in enumerate(lists):
        ids += [m for m, _ in l]
        ds += [d for _, d in l]
        off[v + 1] = len(ids)
    return off, np.array(ids, np.uint32), np.array(ds, np.float32)


def c1_anng():
    return F.read_grp(os.path.join(GOLD, "c1_anng", "grp"))


def duplicated_points():
    """300 copies of one point: every distance is 0, so ids alone order the lists."""
    rs = np.random.RandomState(5)
    lists = [[]]
    for v in range(1, 301):
        others = np.setdiff1d(np.arange(1, 301), [v])
        lists.append([(int(m), 0.0) for m in sorted(rs.choice(others, 80, replace=False))])
    return csr(lists)


def star():
    """Every node points at node 1, whose re-cut list is longer than the one-wave sort takes."""
    n = onng.fast_path_capacity() + 200
    rs = np.random.RandomState(6)
    d = rs.rand(n + 1).astype(np.float32)
    return csr([[], []] + [[(1, float(d[v]))] for v in range(2, n + 1)])


def crafted():
    """Lists of exactly 64 and 65 lower-id entries with higher ids between them, empty lists
    (nodes never inserted or removed), and one list out of distance order."""
    rs = np.random.RandomState(7)
    n = 400
    lists = [[] for _ in range(n)]
    for v in range(1, n):
        if v % 7 == 3:
            continue  # an empty slot
        m = np.setdiff1d(np.arange(1, n), [v] + list(range(3, n, 7)))
        pick = rs.choice(m, min(len(m), 30), replace=False)
        d = np.sort(rs.rand(len(pick)).astype(np.float32))
        lists[v] = [(int(a), float(b)) for a, b in zip(pick, d)]
    full = [a for a in range(1, n) if a % 7 != 3]
    for v, lower in ((300, 64), (301, 65), (302, 129)):
        low = [a for a in full if a < v][:lower]
        high = [a for a in full if a > v][:40]
        ids = low + high
        rs.shuffle(ids)
        d = np.sort(rs.rand(len(ids)).astype(np.float32))
        lists[v] = [(int(a), float(b)) for a, b in zip(ids, d)]
    # node 350: the distance falls at its 12th entry, and its first one is negative zero
    l = lists[350]
    l[0] = (l[0][0], -0.0)
    l[11] = (l[11][0], l[5][1])
    # node 351: out of order at once
    lists[351] = [(12, -1.0), (11, 2.0)]
    return csr(lists)


GRAPHS = {"c1_anng": c1_anng, "duplicated_points": duplicated_points, "star": star, "crafted": crafted}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_recut_equals_the_restatement(name):
    off, ids, ds = GRAPHS[name]()
    longest = int(np.max(np.diff(off.astype(np.int64))))
    for K in KS + (longest + 7,):
        want = D.recut(off, ids, ds, K)
        got = edges.recut(off, ids, ds, K)
        assert np.array_equal(got[0], want[0]), (name, K)
        assert np.array_equal(got[1], want[1]), (name, K)
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (name, K)
    if name == "star":
        assert int(got[0][2] - got[0][1]) > onng.fast_path_capacity()


def test_recut_refuses_what_it_cannot_index():
    off, ids, ds = csr([[], [(2, 1.0)], [(1, 1.0)]])
    with pytest.raises(ngt_amd.NativeError, match="K must be positive"):
        edges.recut(off, ids, ds, 0)
    with pytest.raises(ngt_amd.NativeError, match=r"holds an id outside \[1, 3\)"):
        edges.recut(off, np.array([3, 1], np.uint32), ds, 5)
    with pytest.raises(ngt_amd.NativeError, match=r"holds an id outside \[1, 3\)"):
        edges.recut(off, np.array([2, 0], np.uint32), ds, 5)


# ---- the procedure ---------------------------------------------------------------
@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    """The two indexes of the cases: objects and prf, no graph (the procedure discards it)."""
    d = tmp_path_factory.mktemp("edges")
    return {name: D.make_index(str(d / name), name) for name in ("f16", "u8")}


def read(d, f):
    return open(os.path.join(d, f), "rb").read()


def others(d):
    return {f: read(d, f) for f in sorted(os.listdir(d)) if f != "prf"}


def printed(case):
    """(edge count, accuracy as printed) of `The optimized # of edges=N(acc)`.  The line shows
    six digits of the reference's float, so a returned accuracy is compared through the same six
    digits ("%g" of the float32): the float itself is not recoverable from them (the defaults'
    0.9293097 prints as 0.92931, and the float nearest the decimal 0.92931 is another one)."""
    m = re.match(r"The optimized # of edges=(\d+)\((.*)\)$", CASES[case]["line"])
    return int(m.group(1)), m.group(2)


def last_trace():
    L = ngt_amd.lib()
    samples = (_sigs.EdgeSample * 8)()
    n = ctypes.c_uint32(8)
    assert L.ngt_amd_optimize_edges_last_trace(samples, ctypes.byref(n)) == 0
    return list(samples[:n.value])


def run(case, idx):
    """The returning form on a fresh copy: (edge, accuracy) with the prf and the other files checked."""
    L = ngt_amd.lib()
    before = others(idx)
    err = L.ngt_create_error_object()
    edge, acc = ctypes.c_size_t(0), ctypes.c_float(0.0)
    ok = L.ngt_optimize_number_of_edges_with_result(idx.encode(), D.parameter(CASES[case]["args"]),
                                                    ctypes.byref(edge), ctypes.byref(acc), err)
    msg = base._err_string(L, err)
    L.ngt_destroy_error_object(err)
    assert ok, msg
    assert read(idx, "prf").decode() == CASES[case]["prf"]
    assert others(idx) == before
    return edge.value, np.float32(acc.value)


@pytest.mark.parametrize("case", ["A", "B", "C", "F", "G", "H"])
def test_optimize_number_of_edges_writes_the_reference_prf(case, sources, tmp_path):
    idx = shutil.copytree(sources[CASES[case]["data"]], str(tmp_path / "in"))
    edge, acc = run(case, idx)
    want_edge, want_acc = printed(case)
    assert edge == want_edge
    assert "%g" % acc == want_acc
    trace = last_trace()
    assert len(trace) == 2 and [s.objects for s in trace] == [12500, 25000]
    for s in trace:
        print(case, "sample", s.objects, "edge", s.edge, "accuracy %g" % s.accuracy, "gain %g" % s.gain,
              "maxEpsilon %g" % s.max_epsilon, "guard", s.guard_fired,
              "ms build %.0f recut %.0f search %.0f" % (s.build_ms, s.recut_ms, s.search_ms))
    if case == "C":
        # the reference's runs with the target at each sample's own size (cases D and E) print that
        # sample's values: they need no run of their own
        for s, other in zip(trace, ("D", "E")):
            want_edge, want_acc = printed(other)
            assert ngt_amd.lib().ngt_amd_round_edges(s.edge, 100) == want_edge
            assert "%g" % np.float32(s.accuracy) == want_acc


def test_the_plain_form_and_the_log_line(sources, tmp_path, capfd):
    idx = shutil.copytree(sources["f16"], str(tmp_path / "in"))
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    p = D.parameter(CASES["A"]["args"])
    p.log = True
    ok = L.ngt_optimize_number_of_edges(idx.encode(), p, err)
    msg = base._err_string(L, err)
    L.ngt_destroy_error_object(err)
    assert ok, msg
    assert read(idx, "prf").decode() == CASES["A"]["prf"]
    assert "the optimized number of edges is%d(%s)" % printed("A") in capfd.readouterr().err


@pytest.mark.parametrize("knob", ["NGT_AMD_LA", "NGT_AMD_LAT"])
def test_result_does_not_depend_on_the_search_kernel(knob, sources, tmp_path, monkeypatch):
    monkeypatch.setenv(knob, "0")
    idx = shutil.copytree(sources["f16"], str(tmp_path / "in"))
    edge, acc = run("A", idx)
    assert (edge, "%g" % acc) == printed("A")


def test_device_api_leaves_a_searchable_index():
    """ngt_amd_optimize_edges on an index that has its objects alone: case H's numbers, the
    trace through its own arguments, and afterwards the index searches the last re-cut with the
    last sample's tree -- never a drawn query, never an object no sample took."""
    from ngt_amd.device import DeviceIndex
    rows = D.u8()
    ix = DeviceIndex("l2", "uint8", D.DIM, device=0)
    ix.set_objects(np.vstack([np.zeros((1, D.DIM), np.uint8), rows.astype(np.uint8)]))
    ix.set_search_property(40, 30, 20, 10, 0)
    edge, acc, trace = ix.optimize_edges(num_of_queries=50, num_of_results=20, target_accuracy=0.95,
                                         max_num_of_edges=40)
    want_edge, want_acc = printed("H")
    assert ngt_amd.lib().ngt_amd_round_edges(edge, 40) == want_edge
    assert "%g" % acc == want_acc
    assert [t["objects"] for t in trace] == [12500, 25000]
    assert [k for k, _ in trace[1]["steps"]] == [5, 10, 20, 30][:len(trace[1]["steps"])]
    assert trace[1]["steps"][-1] == (trace[1]["edge"], trace[1]["accuracy"])
    q = rows[:64].astype(np.float32)
    ids, ds, n, _ = ix.search(q, k=5, epsilon=0.1, edge_size=0)
    assert (n == 5).all()
    got = np.unique(ids)
    assert got.min() >= 1 and got.max() <= 25000 + 50
    # at most 50 of the first 64 objects were drawn as queries; every other one finds itself
    assert (ds[:, 0] == 0).sum() >= 64 - 50
    with pytest.raises(ngt_amd.NativeError, match="Too small amount of objects. 25401:100000"):
        ix.optimize_edges(num_of_queries=100000)
    ix.close()


def test_ngtpy_and_cxx_facade(sources, tmp_path):
    want_edge, want_acc = printed("A")
    idx = shutil.copytree(sources["f16"], str(tmp_path / "py"))
    o = ngtpy.Optimizer(log_disabled=True)
    assert o.optimize_number_of_edges_for_anng(idx, num_of_queries=50, num_of_results=20, target_accuracy=0.99,
                                               max_num_of_edges=30) == want_edge
    assert read(idx, "prf").decode() == CASES["A"]["prf"]
    exe = str(tmp_path / "edges_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "edges_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
    idx = shutil.copytree(sources["f16"], str(tmp_path / "cxx"))
    r = subprocess.run([exe, idx] + CASES["A"]["args"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert CASES["A"]["line"] in r.stdout.splitlines()
    assert read(idx, "prf").decode() == CASES["A"]["prf"]


# ---- the thread-local result slots -------------------------------------------------
def in_fresh_thread(f):
    """f() on a new thread, whose result slots start empty; its return value or its exception."""
    import threading
    out = []

    def body():
        try:
            out.append((f(), None))
        except BaseException as e:  # noqa: BLE001 -- handed to the caller's thread
            out.append((None, e))

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if out[0][1] is not None:
        raise out[0][1]
    return out[0][0]


def ask(getter):
    """(status, message) of a *_get_graph entry point, and the 3-row graph it returned."""
    off, ids, ds = np.zeros(4, np.uint64), np.zeros(16, np.uint32), np.zeros(16, np.float32)
    r = getattr(ngt_amd.lib(), getter)(off.ctypes.data, ids.ctypes.data, ds.ctypes.data)
    return r, (ngt_amd.last_error() if r else ""), (off, ids[:int(off[-1])], ds[:int(off[-1])])


def test_a_recut_fills_its_own_result_slot_alone():
    off, ids, ds = csr([[], [(2, 1.0)], [(1, 1.0)]])

    def body():
        got = edges.recut(off, ids, ds, 5)
        return got, ask("ngt_amd_onng_get_graph"), ask("ngt_amd_refine_get_graph"), ask("ngt_amd_recut_get_graph")

    got, o, r, e = in_fresh_thread(body)
    assert o[:2] == (-1, "ngt_amd_onng_get_graph: no reconstructed graph on this thread")
    assert r[:2] == (-1, "ngt_amd_refine_get_graph: no refined graph on this thread")
    assert e[:2] == (0, "")
    want = D.recut(off, ids, ds, 5)
    for a, b, c in zip(e[2], got, want):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(e[2][2].view(np.uint32), want[2].view(np.uint32))


def test_a_failed_reconstruction_clears_its_slot():
    off, ids, ds = csr([[], [(2, 1.0)], [(1, 1.0)]])

    def body():
        onng.reconstruct(off, ids, ds, 1, 1, False)
        first = ask("ngt_amd_onng_get_graph")
        with pytest.raises(ngt_amd.NativeError, match=r"holds an id outside \[1, 3\)"):
            onng.reconstruct(off, np.array([3, 1], np.uint32), ds, 1, 1, False)
        return first, ask("ngt_amd_onng_get_graph")

    first, second = in_fresh_thread(body)
    assert first[:2] == (0, "")
    assert second[:2] == (-1, "ngt_amd_onng_get_graph: no reconstructed graph on this thread")
