"""refine-anng on the device (ngt_amd/csrc/refine.cpp): the list steps against
the plain-Python restatement (tests/refine_restate.py) on synthetic graphs, the
whole refinement against the reference-built fixtures (tests/golden/refine1k),
and ngt_refine_anng end to end through the C API, ngtpy and
NGT/GraphReconstructor.h.  Every comparison is exact: ids, order, distance bits."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import ngt_amd
import oracle_py as O
import refine_data as D
import refine_restate as R
from ngt_amd import base, ngtpy, refine
from ngt_amd.device import DeviceIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = D.F


def same_graph(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2]).view(np.uint32)))


def pad(results, count=None, stride=None):
    """Per-query result lists -> (ids [count][stride], dists, counts)."""
    count = len(results) if count is None else count
    stride = max([len(r) for r in results] + [1]) if stride is None else stride
    ids = np.zeros((count, stride), np.uint32)
    ds = np.zeros((count, stride), np.float32)
    n = np.zeros(count, np.uint32)
    for q, r in enumerate(results):
        n[q] = len(r)
        for j, (i, d) in enumerate(r):
            ids[q, j], ds[q, j] = i, d
    return ids, ds, n


def check_merge(lists, first, results, incoming, **kw):
    csr = R.to_csr(lists)
    ri, rd, rn = pad(results, **kw)
    want = R.merge_csr(*csr, first, ri, rd, rn, incoming)
    got = refine.merge(*csr, first, ri, rd, rn, incoming)
    assert same_graph(got, want)
    return R.from_csr(*got)


# ---- the list steps on a hand-made graph -------------------------------------------
def small_graph():
    """Nodes 1..9; the batch is 3..6.  Lists are in (distance, id) order."""
    return [[],
            [(3, 1.0), (2, 4.0)],                      # 1: holds 3 at 1.0 (incoming from 3 at 1.0 exists)
            [(4, 2.0), (9, 2.5)],                      # 2: holds 4 at 2.0; 4 returns 2 at 1.5: same id above
            [(7, 1.0), (8, 2.0), (9, 3.0)],            # 3: in the batch
            [(2, 2.0), (5, 2.0), (1, 2.0)],            # 4: equal distances (sorted below)
            [],                                        # 5: in the batch, no list
            [(7, 1.0)],                                # 6: in the batch, no results
            [(9, 0.5)],                                # 7: outside the batch
            [],                                        # 8: no list, outside the batch
            [(1, 6.0)]]                                # 9


def small_results():
    return [
        # node 3: itself; 7 again at the stored distance (dropped); 8 at another distance with 7..9
        # between (both stay); 1 (incoming into 1 exists at 1.0); 5 (target in the batch)
        [(3, 0.0), (7, 1.0), (1, 1.0), (5, 1.5), (8, 3.5)],
        # node 4: not itself; ties at 2.0 ordered by id; 2 at 1.5 (node 2 holds 4 at 2.0: skipped);
        # 8 (target with no list, outside the batch)
        [(6, 2.0), (3, 2.0), (2, 1.5), (8, 2.0)],
        # node 5: targets 3 (in the batch, changed by the outgoing step) and 7 (outside)
        [(5, 0.0), (3, 1.5), (7, 0.25)],
        # node 6: nothing found
        [],
    ]


def test_outgoing_and_incoming_on_a_small_graph():
    lists = small_graph()
    lists[4] = sorted(lists[4], key=lambda e: (e[1], e[0]))
    got = check_merge(lists, 3, small_results(), True)
    # 7 once (the adjacent repeat is dropped), 8 twice (9 lies between), never the node itself;
    # 4's edge comes in after the outgoing step, 5's meets the equal entry the step just made
    assert got[3] == [(1, 1.0), (7, 1.0), (5, 1.5), (4, 2.0), (8, 2.0), (9, 3.0), (8, 3.5)]
    assert got[4] == [(2, 1.5), (1, 2.0), (2, 2.0), (3, 2.0), (5, 2.0), (6, 2.0), (8, 2.0)]   # ties by id
    assert got[5] == [(7, 0.25), (3, 1.5)]
    assert got[1] == lists[1]                                               # the edge existed
    assert got[2] == lists[2]                                               # same id at lower_bound: skipped
    assert got[6] == [(7, 1.0), (4, 2.0)]                                   # no results, still a target
    assert got[7] == [(5, 0.25), (9, 0.5), (3, 1.0)] and got[8] == [(4, 2.0), (3, 3.5)]     # outside the batch
    assert got[9] == lists[9]


def test_incoming_off():
    lists = small_graph()
    lists[4] = sorted(lists[4], key=lambda e: (e[1], e[0]))
    got = check_merge(lists, 3, small_results(), False)
    for v in (1, 2, 7, 8, 9):
        assert got[v] == lists[v]


def test_open_candidate_is_inserted_after_an_earlier_insertion_between():
    # node 5 holds (2, 1.5): 2's edge (1.0) meets its own id at lower_bound unless 1's (1.25) went in first
    lists = [[], [], [], [], [], [(2, 1.5), (3, 2.0)]]
    got = check_merge(lists, 1, [[(5, 1.25)], [(5, 1.0)]], True)
    assert got[5] == [(2, 1.0), (1, 1.25), (2, 1.5), (3, 2.0)]
    # the other order of ids: 1's edge is decided first and skipped, 2's does not help it
    lists = [[], [], [], [], [], [(1, 1.5), (3, 2.0)]]
    got = check_merge(lists, 1, [[(5, 1.0)], [(5, 1.25)]], True)
    assert got[5] == [(2, 1.25), (1, 1.5), (3, 2.0)]
    # two open candidates in one list: 3 is let in by 1, 4 has only the higher id 6 between
    lists = [[] for _ in range(8)]
    lists[7] = [(3, 2.0), (4, 5.0)]
    got = check_merge(lists, 1, [[(7, 1.5)], [], [(7, 1.0)], [(7, 3.0)], [], [(7, 4.0)]], True)
    assert got[7] == [(3, 1.0), (1, 1.5), (3, 2.0), (6, 4.0), (4, 5.0)]


def test_last_batch_overhangs_the_rows():
    lists = small_graph()
    lists[4] = sorted(lists[4], key=lambda e: (e[1], e[0]))
    # the block starts at 8 and is 4 wide: rows 10 and 11 do not exist
    res = [[(1, 1.0)], [(8, 0.5), (2, 3.0)], [(1, 1.0)], [(2, 2.0)]]
    got = check_merge(lists, 8, res, True)
    assert got[8] == [(9, 0.5), (1, 1.0)] and (9, 3.0) in got[2] and len(got) == 10
    assert got[1] == [(3, 1.0), (8, 1.0), (2, 4.0)]              # nothing from the queries past the rows


def test_bad_results_are_errors():
    csr = R.to_csr(small_graph()[:4] + [[]] * 6)
    for bad in (0, 10, 0xFFFFFFFF):
        ri, rd, rn = pad([[(bad, 1.0)]])
        with pytest.raises(ngt_amd.NativeError, match="query 3 is an id outside"):
            refine.merge(*csr, 3, ri, rd, rn, True)
    ri, rd, rn = pad([[(1, 1.0)]])
    rn[0] = 2
    with pytest.raises(ngt_amd.NativeError, match="more results than the stride"):
        refine.merge(*csr, 3, ri, rd, rn, True)
    with pytest.raises(ngt_amd.NativeError, match="first id"):
        refine.merge(*csr, 10, ri, rd, rn, True)


# ---- random graphs: ties, repeats at other distances, many workgroups ------------------
@pytest.fixture(scope="module")
def random_case():
    """2,500 nodes, distances from five values and not symmetric, so results
    meet their own id at other distances all the time; a batch of 700."""
    n, deg, k = 2500, 12, 9
    rng = np.random.default_rng(5)
    lists = [[]]
    for v in range(1, n + 1):
        nb = [int(u) for u in rng.choice(np.arange(1, n + 1), deg, replace=False) if u != v]
        lists.append(sorted(((u, float(rng.integers(1, 6))) for u in nb), key=lambda e: (e[1], e[0])))
    for v in (1, 400, 401, 1100, n):
        lists[v] = []
    first, count = 350, 700
    results = []
    for q in range(count):
        v = first + q
        own = [e[0] for e in lists[v][:4]]                       # some are in the list already
        new = [int(u) for u in rng.choice(np.arange(1, n + 1), k, replace=False)]
        ids = list(dict.fromkeys(own + new + ([v] if q % 3 == 0 else [])))[:k + 4]
        if q % 50 == 7:
            ids = []
        # its neighbours keep pointing back at it: incoming edges that exist, at this or another distance
        results.append([(u, float(rng.integers(1, 6))) for u in ids])
    for q in range(0, count, 5):                                  # the reverse edge exists at the same distance
        v = first + q
        for u, d in results[q][:3]:
            if u != v and all(e[0] != v for e in lists[u]):
                lists[u] = sorted(lists[u] + [(v, d)], key=lambda e: (e[1], e[0]))
    return lists, first, results


def test_random_graph_with_ties_and_repeats(random_case):
    lists, first, results = random_case
    got = check_merge(lists, first, results, True)
    assert any(len(set(e[0] for e in l)) != len(l) for l in got)      # an id twice in one list
    check_merge(lists, first, results, False)
    # the same block cut by the end of the rows
    cut = first + 300
    check_merge([[e for e in l if e[0] < cut] for l in lists[:cut]], first,
                [[e for e in r if e[0] < cut] for r in results], True)


def test_merge_is_deterministic(random_case):
    lists, first, results = random_case
    csr = R.to_csr(lists)
    ri, rd, rn = pad(results)
    a = refine.merge(*csr, first, ri, rd, rn, True, with_stats=True)
    b = refine.merge(*csr, first, ri, rd, rn, True, with_stats=True)
    assert same_graph(a, b)
    for k in ("launches", "candidates", "edges_out", "longest_list"):
        assert a[3][k] == b[3][k], k


# ---- lists above the capacity of the one-wave sort ---------------------------------------
def test_target_one_past_the_fast_path_capacity():
    cap = refine.fast_path_capacity()
    assert cap == 1024
    count = cap + 1
    n = count + 3
    hub, outside = 5, n - 1                 # one target inside the batch, one outside
    lists = [[] for _ in range(n)]
    lists[2] = [(hub, 1.0)]
    rng = np.random.default_rng(3)
    results = []
    for q in range(count):
        v = 1 + q
        r = [(outside, float(rng.integers(1, 40)))]
        if v != hub:
            r.append((hub, float(rng.integers(1, 40))))
        results.append(r)
    got = check_merge(lists, 1, results, True)
    assert len(got[outside]) == cap + 1 and len(got[hub]) >= cap
    # a batch node whose own list and results together pass the capacity
    lists = [[] for _ in range(cap + 40)]
    lists[3] = [(u, float(u)) for u in range(4, cap + 2)]
    res = [[], [], [(u, float(u) + 1.5) for u in range(4, 24)]]     # each lands behind another id: all stay
    got = check_merge(lists, 1, res, True)
    assert len(got[3]) == cap - 2 + 20


def test_prune():
    lists = small_graph()
    lists[4] = sorted(lists[4], key=lambda e: (e[1], e[0]))
    csr = R.to_csr(lists)
    for k in (1, 2, 3, 100):
        assert same_graph(refine.prune(*csr, k), R.prune_csr(*csr, k))
    assert [len(l) for l in R.from_csr(*refine.prune(*csr, 2))] == [0, 2, 2, 2, 2, 0, 1, 1, 0, 1]


# ---- the whole refinement on a device index ---------------------------------------------
def epsilon_of(name):
    eps, acc = D.CASES[name][:2]
    if acc > 0.0:
        table = ngtpy.accuracy_table(os.path.join(D.REFINE1K, D.CASES[name][5]))
        return ngtpy.epsilon_from_expected_accuracy(table, float(np.float32(acc)))
    return eps


@pytest.fixture(scope="module")
def device_index():
    prop, rows, valid, tree = D.index_parts()
    ix = DeviceIndex("l2", "float", 128, device=0)
    ix.set_objects(rows, valid)
    ix.set_tree(tree)
    ix.set_search_property(int(prop["EdgeSizeForSearch"]), int(prop["DynamicEdgeSizeBase"]),
                           int(prop["DynamicEdgeSizeRate"]), int(prop["SeedSize"]), 0)
    yield ix
    ix.close()


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_device_index_equals_reference(device_index, name):
    _, _, k, explore, batch, src = D.CASES[name]
    creation = int(D.index_parts()[0]["EdgeSizeForCreation"])
    args = (epsilon_of(name), k, creation, -1 if explore == D.INT_MIN else explore, batch)
    a = refine.refine_anng(device_index, *D.csr(src), *args, with_stats=True)
    assert same_graph(a, D.csr(name))
    b = refine.refine_anng(device_index, *D.csr(src), *args, with_stats=True)
    assert same_graph(a, b)
    for key in ("launches", "batches", "searched", "candidates", "edges_out", "longest_list"):
        assert a[3][key] == b[3][key], key
    assert a[3]["batches"] == -(-1000 // batch) and a[3]["searched"] == 1000


def test_device_index_errors_keep_the_input_graph(device_index):
    prop, rows, _, tree = D.index_parts()
    off, ids, d = D.csr("anng")
    with pytest.raises(ngt_amd.NativeError, match="Invalid edge size parameters -3"):
        refine.refine_anng(device_index, off, ids, d, 0.0, 0, 20, -3, 256)
    with pytest.raises(ngt_amd.NativeError, match="batch size is 0"):
        refine.refine_anng(device_index, off, ids, d, 0.0, 0, 20, -1, 0)
    # a size no search launch can hold fails cleanly after the graph was handed to the index ...
    with pytest.raises(ngt_amd.NativeError, match="LDS"):
        refine.refine_anng(device_index, off, ids, d, 0.0, -100000, 20, -1, 256)
    # ... and the index searches the input graph again
    q = rows[1:5]
    gi, gd, gn, _ = device_index.search(q[:, :128], k=10, epsilon=0.1, seed_mode=0)
    for i in range(len(q)):
        seeds, _, _ = O.tree_seeds("l2", tree, q[i], 10, int(prop["SeedSize"]))
        oid, od, _ = O.search("l2", rows, off, ids, q[i], seeds, 10, np.float32(0.1), edge_size=2 ** 31 - 1)
        assert list(gi[i, :gn[i]]) == list(oid) and np.array_equal(gd[i, :gn[i]].view(np.uint32), od.view(np.uint32))


# ---- end to end ------------------------------------------------------------------------------
def check_output(out, name, src_dir):
    assert filecmp.cmp(os.path.join(out, "grp"), os.path.join(D.REFINE1K, name, "grp"), shallow=False)
    for f in ("prf", "obj", "tre"):
        assert filecmp.cmp(os.path.join(out, f), os.path.join(src_dir, f), shallow=False), f
    assert sorted(os.listdir(out)) == ["grp", "obj", "prf", "tre"]


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_refine_anng_capi(name, tmp_path):
    eps, acc, k, explore, batch, src = D.CASES[name]
    src_dir = D.make_index_dir(str(tmp_path / "in"), src)
    L = ngt_amd.lib()
    ix = base.Index(src_dir)
    assert L.ngt_refine_anng(ix.index, eps, acc, k, explore, batch, ix.err), base._err_string(L, ix.err)
    out = str(tmp_path / "out")
    ix.save(out)
    check_output(out, name, src_dir)
    if name == "r_b256":
        # searches on the same handle see the refined graph
        prop, rows, _, tree = D.index_parts()
        offs, ids, _ = D.csr(name)
        qs = np.load(os.path.join(D.GOLD, "queries.npy")).astype(np.float32)[:16]
        gi, gd, gn = ix.batch_search(qs, 10, 0.05)
        for i, q in enumerate(qs):
            seeds, _, _ = O.tree_seeds("l2", tree, q, 10, int(prop["SeedSize"]))
            oid, od, _ = O.search("l2", rows, offs, ids, q, seeds, 10, np.float32(0.05), edge_size=2 ** 31 - 1)
            assert list(gi[i, :gn[i]]) == list(oid), i
            assert np.array_equal(gd[i, :gn[i]].view(np.uint32), od.view(np.uint32)), i
    ix.close()


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_refine_anng_ngtpy(name, tmp_path):
    eps, acc, k, explore, batch, src = D.CASES[name]
    work = D.make_index_dir(str(tmp_path / "ix"), src)
    keep = D.make_index_dir(str(tmp_path / "keep"), src)
    ix = ngtpy.Index(work)
    ix.refine_anng(epsilon=eps, expected_accuracy=acc, num_of_edges=k, num_of_explored_edges=explore,
                   batch_size=batch)
    ix.save()
    ix.close()
    check_output(work, name, keep)


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("refine_cxx") / "refine_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "refine_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
    return exe


CLI = {"r_b256": ["-e", "0.0", "-b", "256"], "r_one": ["-e", "0.0"], "r_k10": ["-e", "0.0", "-k", "10", "-b", "100"],
       "r_k30": ["-e", "0.0", "-k", "30", "-b", "256"], "r_km30": ["-e", "0.0", "-k", "-30", "-b", "256"],
       "r_E10": ["-e", "-0.1", "-E", "10", "-b", "256"], "r_a": ["-a", "0.8", "-b", "256"]}


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_refine_anng_cxx(sample, name, tmp_path):
    src_dir = D.make_index_dir(str(tmp_path / "in"), D.CASES[name][5])
    out = str(tmp_path / "out")
    r = subprocess.run([sample] + CLI[name] + [src_dir, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    check_output(out, name, src_dir)


def test_errors_leave_the_handle_as_it_was(sample, tmp_path):
    src_dir = D.make_index_dir(str(tmp_path / "in"))
    L = ngt_amd.lib()
    ix = base.Index(src_dir)
    assert not L.ngt_refine_anng(ix.index, 0.1, 0.8, 0, D.INT_MIN, 256, ix.err)
    assert ("GraphReconstructor::refineANNG: AccuracyTable: The accuracy table is not set yet. The table size=0"
            in base._err_string(L, ix.err))
    assert not L.ngt_refine_anng(ix.index, 0.1, 0.0, 0, -3, 256, ix.err)
    assert "Invalid edge size parameters" in base._err_string(L, ix.err)
    # a size above what a search launch holds: the device call fails after it took the graph
    assert not L.ngt_refine_anng(ix.index, 0.1, 0.0, -100000, D.INT_MIN, 256, ix.err)
    assert "LDS" in base._err_string(L, ix.err)
    out = str(tmp_path / "out")
    ix.save(out)
    assert filecmp.cmp(os.path.join(out, "grp"), os.path.join(src_dir, "grp"), shallow=False)
    # and the handle still refines
    assert L.ngt_refine_anng(ix.index, 0.0, 0.0, 10, D.INT_MIN, 100, ix.err), base._err_string(L, ix.err)
    ix.save(out)
    assert filecmp.cmp(os.path.join(out, "grp"), os.path.join(D.REFINE1K, "r_k10", "grp"), shallow=False)
    ix.close()
    r = subprocess.run([sample, "-E", "-3", src_dir, str(tmp_path / "no")], capture_output=True, text=True)
    assert r.returncode == 1 and "Invalid edge size parameters" in r.stderr and not os.path.exists(str(tmp_path / "no"))
