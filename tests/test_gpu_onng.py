"""ONNG reconstruction on the device (ngt_amd/csrc/onng.cpp): the device call
against the reference-built fixtures (tests/golden/onng2k) and, on synthetic
graphs, against the plain-Python restatement (tests/onng_restate.py); and
ngt_optimizer_execute end to end through the C API, ngtpy.Optimizer and
NGT/GraphOptimizer.h.  Every comparison is exact: ids, order, distance bits."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import ngt_amd
import ngt_files as F
import onng_data as D
import onng_restate as R
import oracle_py as O
from ngt_amd import base, ngtpy, onng

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_graph(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2]).view(np.uint32)))


def check_against_restatement(csr, o, i, path, min_edges=0, input_is_anng=True):
    want = R.reconstruct(csr[0], csr[1], csr[2], o, i, path, min_edges, input_is_anng)
    got = onng.reconstruct(csr[0], csr[1], csr[2], o, i, path, min_edges, input_is_anng)
    assert same_graph(got, want)
    return got


# ---- fixtures -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_device_equals_reference(name):
    o, i, path, min_edges, src = D.CASES[name]
    off, ids, d = D.csr(src)
    got = onng.reconstruct(off, ids, d, o, i, path, min_edges, input_is_anng=(src == "anng"))
    assert same_graph(got, D.csr(name))


@pytest.mark.parametrize("o,i", [(0, 40), (5, 0)])
def test_device_without_outgoing_or_incoming(o, i):
    check_against_restatement(D.csr("anng"), o, i, False)
    check_against_restatement(D.csr("onng_S"), o, i, False, input_is_anng=False)


def test_device_is_deterministic():
    off, ids, d = D.csr("anng")
    a = onng.reconstruct(off, ids, d, 5, 40, True, with_stats=True)
    b = onng.reconstruct(off, ids, d, 5, 40, True, with_stats=True)
    assert same_graph(a, b) and same_graph(a, D.csr("onng_S"))
    # the number of launches depends on the graph alone, not on scheduling
    for k in ("candidates", "phase_b_launches", "max_passes_per_rank", "ranks"):
        assert a[3][k] == b[3][k], k
    assert a[3]["candidates"] == 402123


# ---- end to end -------------------------------------------------------------------
def _check_output(out, anng):
    assert filecmp.cmp(os.path.join(out, "grp"), os.path.join(D.ONNG2K, "onng_S", "grp"), shallow=False)
    want = F.read_prf(os.path.join(D.ONNG2K, "onng_S", "prf"))
    assert want["GraphType"] == "ONNG"
    assert F.read_prf(os.path.join(out, "prf")) == want
    for f in ("obj", "tre"):
        assert filecmp.cmp(os.path.join(out, f), os.path.join(anng, f), shallow=False), f
    assert sorted(os.listdir(out)) == ["grp", "obj", "prf", "tre"]


@pytest.fixture(scope="module")
def anng_dir(tmp_path_factory):
    return D.make_anng_dir(str(tmp_path_factory.mktemp("onng") / "anng"))


def test_optimizer_execute_capi(anng_dir, tmp_path):
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    opt = L.ngt_create_optimizer(True, err)
    out = str(tmp_path / "onng")
    assert L.ngt_optimizer_set_minimum(opt, 5, 40, -1, -1, err)
    assert L.ngt_optimizer_set_processing_modes(opt, False, False, False, err)
    assert L.ngt_optimizer_execute(opt, anng_dir.encode(), out.encode(), err), base._err_string(L, err)
    L.ngt_destroy_optimizer(opt)
    L.ngt_destroy_error_object(err)
    _check_output(out, anng_dir)
    # the result opens and searches like any index: 16 queries against the oracle
    prop = F.read_prf(os.path.join(out, "prf"))
    rows, _ = F.read_obj(os.path.join(out, "obj"), 128, np.float32)
    offs, ids, _ = F.read_grp(os.path.join(out, "grp"))
    tree = F.read_tre(os.path.join(out, "tre"), 128, np.float32)
    qs = np.load(os.path.join(D.GOLD, "queries.npy")).astype(np.float32)[:16]
    ix = base.Index(out)
    gi, gd, gn = ix.batch_search(qs, 10, 0.05)
    for i, q in enumerate(qs):
        seeds, _, _ = O.tree_seeds("l2", tree, q, 10, int(prop["SeedSize"]))
        oid, od, _ = O.search("l2", rows, offs, ids, q, seeds, 10, np.float32(0.05),
                              edge_size=int(prop["EdgeSizeForSearch"]))
        assert list(gi[i, :gn[i]]) == list(oid), i
        assert np.array_equal(gd[i, :gn[i]].view(np.uint32), od.view(np.uint32)), i
    ix.close()


def test_optimizer_execute_ngtpy(anng_dir, tmp_path):
    out = str(tmp_path / "onng")
    opt = ngtpy.Optimizer(num_of_outgoings=5, num_of_incomings=40, log_disabled=True)
    opt.set_processing_modes(True, False, False, False)
    opt.execute(anng_dir, out)
    _check_output(out, anng_dir)
    # path adjustment alone leaves the prf's GraphType as it was
    out_p = str(tmp_path / "onng_P")
    opt.set(num_of_outgoings=0, num_of_incomings=0)
    opt.execute(anng_dir, out_p)
    assert filecmp.cmp(os.path.join(out_p, "grp"), os.path.join(D.ONNG2K, "onng_P", "grp"), shallow=False)
    assert filecmp.cmp(os.path.join(out_p, "prf"), os.path.join(anng_dir, "prf"), shallow=False)


def test_optimizer_execute_cxx(anng_dir, tmp_path):
    exe = str(tmp_path / "onng_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "onng_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
    out = str(tmp_path / "onng")
    r = subprocess.run([exe, anng_dir, out, "5", "40", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _check_output(out, anng_dir)
    out_e = str(tmp_path / "onng_E")
    r = subprocess.run([exe, anng_dir, out_e, "5", "40", "12"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert filecmp.cmp(os.path.join(out_e, "grp"), os.path.join(D.ONNG2K, "onng_E", "grp"), shallow=False)
    r = subprocess.run([exe, anng_dir, str(tmp_path / "no"), "5", "40", "0", "tuning"], capture_output=True, text=True)
    assert r.returncode == 1 and "set_processing_modes" in r.stderr and not os.path.exists(str(tmp_path / "no"))


# ---- synthetic graphs (path adjustment reads only the stored distances) -----------
def csr_of(lists):
    """lists: per node id (slot 0 the dummy) a list of (id, distance)."""
    return R.to_csr(lists)


def chain(ascending):
    # ids: 1 the filler F, 2 the far node X, then v_1 .. v_40
    n = 40
    vid = [3 + k if ascending else 3 + (n - 1 - k) for k in range(n)]
    lists = [[] for _ in range(n + 3)]
    lists[vid[0]] = [(1, 0.5), (2, 1.0)]                     # F has no edge to X
    for k in range(1, n):
        lists[vid[k]] = [(vid[k - 1], 1.0), (2, float(k + 1))]  # x_k = k + 1
    return lists, vid


def test_ascending_chain_alternates():
    lists, vid = chain(True)
    st = {}
    want = R.path_adjustment(lists, 0, st)
    assert st["depth"] >= 8
    kept_x = [any(u == 2 for u, _ in want[v]) for v in vid]
    assert kept_x == [k % 2 == 0 for k in range(40)]
    off, ids, d, stats = onng.reconstruct(*csr_of(lists), 0, 0, True, with_stats=True)
    assert same_graph((off, ids, d), R.to_csr(want))
    assert stats["max_passes_per_rank"] >= 8


def test_descending_chain_keeps_every_edge():
    lists, _ = chain(False)
    want = R.path_adjustment(lists, 0)
    assert want == lists
    off, ids, d, stats = onng.reconstruct(*csr_of(lists), 0, 0, True, with_stats=True)
    assert same_graph((off, ids, d), csr_of(lists))
    assert stats["max_passes_per_rank"] == 1


@pytest.fixture(scope="module")
def hub_graph():
    """Points in the plane, each with its 6 nearest neighbours and the hub
    (node 1); one more node than twice the fast-path capacity would need."""
    cap = onng.fast_path_capacity()
    n = cap + 90
    rng = np.random.default_rng(7)
    pts = rng.random((n + 1, 2)).astype(np.float32)
    diff = pts[:, None, :] - pts[None, :, :]
    dist = np.sqrt((diff * diff).sum(-1, dtype=np.float32)).astype(np.float32)   # symmetric bit for bit
    lists = [[], []]
    for v in range(2, n + 1):
        dv = dist[v].copy()
        dv[[0, v]] = np.inf
        nb = set(np.argsort(dv, kind="stable")[:6].tolist()) | {1}
        lists.append(sorted(((int(u), float(dist[v, u])) for u in nb), key=lambda e: (e[1], e[0])))
    lists[1] = sorted(((int(u), float(dist[1, u])) for u in range(2, 8)), key=lambda e: (e[1], e[0]))
    return cap, lists


def test_hub_longer_than_the_fast_path(hub_graph):
    cap, lists = hub_graph
    adjusted = R.edge_adjustment(lists, lists, 3, 8)
    assert len(adjusted[1]) > cap                      # in-degree of the hub, and tmp[hub] of path adjustment
    assert max(len(l) for l in adjusted[2:]) <= cap
    check_against_restatement(csr_of(lists), 3, 8, True)
    check_against_restatement(csr_of(lists), 3, 8, False)
    # the hub list as the input of a conversion and of path adjustment alone
    check_against_restatement(csr_of(adjusted), 4, 6, True, input_is_anng=False)
    check_against_restatement(csr_of(adjusted), 0, 0, True)


@pytest.fixture(scope="module")
def tie_graph():
    """300 nodes, symmetric distances drawn from four integer values."""
    n = 300
    rng = np.random.default_rng(11)
    w = rng.integers(1, 5, size=(n + 1, n + 1))
    w = np.minimum(w, w.T).astype(np.float64)
    lists = [[]]
    for v in range(1, n + 1):
        nb = [int(u) for u in rng.choice(np.arange(1, n + 1), 14, replace=False) if u != v]
        lists.append(sorted(((u, float(w[v, u])) for u in nb), key=lambda e: (e[1], e[0])))
    return lists


def test_ties(tie_graph):
    csr = csr_of(tie_graph)
    got = check_against_restatement(csr, 4, 10, True)
    assert len(got[1]) < len(R.reconstruct(*csr, 4, 10, False)[1])       # paths were found
    check_against_restatement(csr, 0, 0, True)
    check_against_restatement(csr, 6, 6, True, input_is_anng=False)


def test_min_edges_guard_turns_false_within_lists(tie_graph):
    csr = csr_of(tie_graph)
    tmp = R.from_csr(*R.reconstruct(*csr, 4, 10, False))
    free = R.path_adjustment(tmp, 0)
    for min_edges in (9, 15):
        guarded = R.path_adjustment(tmp, min_edges)
        # some list lost edges while the guard held and kept the rest once it did not
        assert any(len(f) < len(g) == min_edges < len(t) for f, g, t in zip(free, guarded, tmp))
        got = onng.reconstruct(*csr, 4, 10, True, min_edges)
        assert same_graph(got, R.to_csr(guarded))


def test_repeated_id_is_an_error():
    lists = [[], [(2, 1.0), (3, 2.0)], [(1, 1.0)], [(1, 1.0), (2, 2.0), (1, 3.0)], []]
    with pytest.raises(R.RepeatedId):
        R.path_adjustment(lists, 0)
    with pytest.raises(ngt_amd.NativeError, match="node 3 repeats an id"):
        onng.reconstruct(*csr_of(lists), 0, 0, True)
    # edge adjustment alone takes such lists
    check_against_restatement(csr_of(lists), 2, 2, False)


def test_unsorted_list_is_an_error_for_path_adjustment_alone():
    lists = [[], [(2, 2.0), (3, 1.0)], [(1, 2.0)], [(1, 1.0)]]
    with pytest.raises(ngt_amd.NativeError, match="node 1 is not"):
        onng.reconstruct(*csr_of(lists), 0, 0, True)
    check_against_restatement(csr_of(lists), 1, 2, True)       # edge adjustment sorts


def test_nodes_without_a_list(tie_graph):
    lists = [list(l) for l in tie_graph]
    for v in (1, 7, 150, 299, 300):            # empty lists that other nodes still point to
        lists[v] = []
    lists += [[], []]                          # rows nobody points to
    csr = csr_of(lists)
    check_against_restatement(csr, 4, 10, True)
    check_against_restatement(csr, 0, 10, True, input_is_anng=False)
    # only the dummy slot, and no edges at all
    empty = (np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    assert same_graph(onng.reconstruct(*empty, 10, 120, True), empty)


@pytest.mark.parametrize("bad", [0, 4, 0xFFFFFFFF])
def test_id_of_no_row_is_an_error(bad):
    lists = [[], [(2, 1.0)], [(1, 1.0), (3, 2.0)], [(2, 2.0)]]
    off, ids, d = csr_of(lists)
    ids = ids.copy()
    ids[2] = bad
    with pytest.raises(ngt_amd.NativeError, match="node 2 holds an id outside"):
        onng.reconstruct(off, ids, d, 1, 1, True)
