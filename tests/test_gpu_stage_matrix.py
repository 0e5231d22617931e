"""refine-anng, object removal and the ONNG reconstruction on the device across
the construction cases of tests/build_data.py: L1, L2, Hamming, Jaccard,
Cosine, Normalized Cosine and Angle, float and uint8 rows, heavy distance ties
and 30 % duplicate rows.  Each stage starts from the index the reference built
(tests/golden/build_<case>/ plus the written obj, stage_matrix.make_index_dir),
runs through the C API -- ngt_refine_anng, ngt_batch_remove_index /
ngt_remove_index, ngt_optimizer_execute -- and is compared byte for byte with
the files the reference CLI wrote for the same input (tests/golden/stage_<case>/,
stage_matrix.json, make_stage_matrix_goldens.py).  A grp mismatch is reported
as the first node that differs.  tests/test_stage_matrix_host.py holds what
each fixture has to contain.  Every table has 2,001 rows."""
import os

import numpy as np
import pytest

import ngt_amd
import ngt_files as F
import oracle_py as O
import search_matrix as S
import stage_matrix as M
from ngt_amd import NativeError, base, refine
from ngt_amd.device import DeviceIndex
from test_gpu_build_matrix import first_graph_difference, first_tree_difference

pytestmark = pytest.mark.gpu


def read(d, f):
    return open(os.path.join(d, f), "rb").read()


def assert_grp(out, name, stage):
    got, want = read(out, "grp"), M.fixture_bytes(name, stage, "grp")
    if got != want:
        pytest.fail("%s %s grp: %s" % (name, stage, first_graph_difference(got, want)))


def assert_tre(out, name):
    c = S.load(name)
    got, want = read(out, "tre"), M.fixture_bytes(name, "remove", "tre")
    if got != want:
        pytest.fail("%s remove tre: %s" % (name, first_tree_difference(got, want, c.dim, c.dtype)))


def assert_unchanged(out, src, files):
    for f in files:
        assert read(out, f) == read(src, f), f
    assert sorted(os.listdir(out)) == ["grp", "obj", "prf", "tre"]


def refine_anng(ix, args):
    L = ix._L
    assert L.ngt_refine_anng(ix.index, *args, ix.err), base._err_string(L, ix.err)


# ---- refine-anng ------------------------------------------------------------------------
def refine_through_the_capi(name, stage, args, tmp_path):
    src = M.make_index_dir(name, str(tmp_path / "in"))
    ix = base.Index(src)
    try:
        refine_anng(ix, args)
        out = str(tmp_path / "out")
        ix.save(out)
    finally:
        ix.close()
    assert_grp(out, name, stage)
    assert_unchanged(out, src, ("prf", "obj", "tre"))


@pytest.mark.parametrize("name", M.CASES)
def test_refine_a_capi(name, tmp_path):
    """Epsilon 0.1, eight batches of 256, incoming edges: the searches take the
    stored rows -- uint8, normalised or not -- as prepared queries."""
    refine_through_the_capi(name, "refine_a", M.REFINE_A[1], tmp_path)


@pytest.mark.parametrize("name", M.REFINE_B_CASES)
def test_refine_b_capi(name, tmp_path):
    """15 results per search (above EdgeSizeForCreation), no incoming edges, lists pruned to 15."""
    refine_through_the_capi(name, "refine_b", M.REFINE_B[1], tmp_path)


@pytest.mark.parametrize("name", M.CASES)
def test_refine_a_device_index(name):
    """The same refinement on a DeviceIndex loaded with rows, graph and tree."""
    c = S.load(name)
    eps, _, k, _, batch = M.REFINE_A[1]
    ix = DeviceIndex(c.metric, "float" if c.otype == "f" else "uint8", c.dim)
    try:
        ix.set_objects(c.rows)
        ix.set_tree(c.tree)
        ix.set_search_property(int(c.prop["EdgeSizeForSearch"]), int(c.prop["DynamicEdgeSizeBase"]),
                               int(c.prop["DynamicEdgeSizeRate"]), int(c.prop["SeedSize"]), 0)
        got = refine.refine_anng(ix, *M.graph(name, "build"), eps, k, int(c.prop["EdgeSizeForCreation"]), -1, batch)
    finally:
        ix.close()
    woffs, wids, wds = M.graph(name, "refine_a")
    offs, ids, ds = got
    assert len(offs) == len(woffs)
    for v in range(1, len(offs) - 1):
        a, b, lo, hi = int(offs[v]), int(offs[v + 1]), int(woffs[v]), int(woffs[v + 1])
        assert list(ids[a:b]) == list(wids[lo:hi]), (name, "node", v)
        assert ds[a:b].tobytes() == wds[lo:hi].tobytes(), (name, "node", v)


@pytest.mark.parametrize("knob", ["NGT_AMD_LA", "NGT_AMD_LAT"])
def test_refined_graph_does_not_depend_on_the_search_kernel(knob, tmp_path, monkeypatch):
    """l2_f20's rows are padded to 32 elements, which no lookahead kernel takes
    (search_plan.cpp: L2 float rows of 96 or 128), so on it the knob only shows
    that it leaves the one-expansion kernel's result alone.  The kernels the
    knobs do switch off are reached by the 128-element rows of refine1k: its
    r_b256 graph is the reference's with either of them off."""
    import filecmp

    import refine_data as RD
    monkeypatch.setenv(knob, "0")
    refine_through_the_capi("l2_f20", "refine_a", M.REFINE_A[1], tmp_path / "l2_f20")
    src = RD.make_index_dir(str(tmp_path / "refine1k"))
    ix = base.Index(src)
    try:
        refine_anng(ix, RD.CASES["r_b256"][:5])
        out = str(tmp_path / "refine1k_out")
        ix.save(out)
    finally:
        ix.close()
    assert filecmp.cmp(os.path.join(out, "grp"), os.path.join(RD.REFINE1K, "r_b256", "grp"), shallow=False)


# ---- removal ----------------------------------------------------------------------------
def assert_removed_files(out, name, src):
    e = M.expected()[name]["remove"]
    assert_grp(out, name, "remove")
    assert_tre(out, name)
    assert M.sha256(read(out, "obj")) == e["obj_sha256"]
    assert_unchanged(out, src, ("prf",))


def assert_answers_after_removal(live, saved, name):
    """The handle that removed and the index it saved, reopened, answer
    ngt_batch_search_index like the oracle on the reference's removed graph and
    tree: the same ids and distance bits, no removed id.  A query whose leaf the
    removal emptied has no tree seeds and takes getSeedsFromGraph's random ones
    (Index.h:1145-1155) from the library's rand() stream, here after srand(1);
    it comes back with k results like every other query."""
    c = S.load(name)
    valid = M.valid_after_removal(name)
    offs, ids, _ = M.graph(name, "remove")
    graph_empty = np.diff(offs.astype(np.int64)) == 0
    tree = M.removed_tree(name)
    again = base.Index(saved)
    try:
        for k, eps in ((10, 0.1), (50, 0.02)):
            answers = []
            for ix in (live, again):
                ngt_amd.lib().ngt_amd_srand(1)
                answers.append(ix.batch_search(c.queries, k=k, epsilon=eps))
            rand = M.glibc_rand(1)
            for i, q in enumerate(c.oq):
                seeds, _, _ = O.tree_seeds(c.metric, tree, q, k, c.seed_size, c.dtype)
                fallback = len(seeds) == 0
                if fallback:
                    seeds = np.array(M.random_seeds(rand, graph_empty, c.seed_size), np.uint32)
                oid, od, _ = O.search(c.metric, c.rows, offs, ids, q, seeds, k, np.float32(eps), edge_size=c.edge_size)
                assert not fallback or len(oid) == k, (name, k, i)
                assert valid[oid].all(), (name, k, i)
                for gi, gd, gn in answers:
                    n = int(gn[i])
                    assert n == len(oid), (name, k, i, n, len(oid))
                    assert list(gi[i, :n]) == list(oid), (name, k, i)
                    assert gd[i, :n].tobytes() == od.tobytes(), (name, k, i)
    finally:
        again.close()


def test_emptied_leaf_seeds_in_query_order_and_one_query_at_a_time(tmp_path):
    """remove1k's rm_oneleaf empties leaf 22 of an L2 float index of 128 elements,
    the shape ngt_search_index would hand to the resident serving grid, whose
    in-kernel descent has no fallback: a tree with an empty leaf is not served.
    The first removed row descends to that leaf.  k = 3 with epsilon -0.2 keeps
    what the seeds reach, so three getRandomSeeds draws after srand(1) give three
    different answers: a batch holding the query three times, a seeded query in
    between, takes them in query order, and so do three single-query calls."""
    import refine_restate as R
    import remove_data as RD
    e = RD.expected()["rm_oneleaf"]
    rows, _, _, _, _, _, prop = RD.load_input("anng")
    offs, ids, _ = F.read_grp(os.path.join(RD.RM, "rm_oneleaf", "grp"))
    tree = F.read_tre(os.path.join(RD.RM, "rm_oneleaf", "tre"), 128, np.float32)
    graph_empty = np.diff(offs.astype(np.int64)) == 0
    k, eps, seed_size = 3, -0.2, int(prop["SeedSize"])
    es = R.edge_size(prop, None, eps)
    gone, other = e["ids"][0], 1
    assert other not in e["ids"]
    assert len(O.tree_seeds("l2", tree, rows[gone], k, seed_size)[0]) == 0

    def oracle(row, seeds):
        return O.search("l2", rows, offs, ids, rows[row], np.asarray(seeds, np.uint32), k, np.float32(eps), edge_size=es)[:2]

    rand = M.glibc_rand(1)
    want = [oracle(gone, M.random_seeds(rand, graph_empty, seed_size)) for _ in range(3)]
    assert len({tuple(w[0]) for w in want}) == 3 and all(len(w[0]) == k for w in want)
    seeded = oracle(other, O.tree_seeds("l2", tree, rows[other], k, seed_size)[0])

    ix = base.Index(RD.copy_input("anng", str(tmp_path / "in")))
    try:
        assert ix.batch_remove(e["ids"]).all()
        q = rows[[gone, other, gone, gone], :128]
        ngt_amd.lib().ngt_amd_srand(1)
        gi, gd, gn = ix.batch_search(q, k=k, epsilon=eps)
        for i, (oid, od) in enumerate([want[0], seeded, want[1], want[2]]):
            assert int(gn[i]) == len(oid) and list(gi[i, :gn[i]]) == list(oid), i
            assert gd[i, :gn[i]].tobytes() == od.tobytes(), i
        ngt_amd.lib().ngt_amd_srand(1)
        for i, (oid, od) in enumerate(want):
            r = ix.search(rows[gone, :128].astype(np.float64), k, eps)
            assert [x.id for x in r] == list(oid), i
            assert np.array([x.distance for x in r], np.float32).tobytes() == od.tobytes(), i
    finally:
        ix.close()


@pytest.mark.parametrize("name", M.CASES)
def test_batch_remove(name, tmp_path):
    """The hub, its first neighbours, a whole leaf and, where there are any, a
    row with a live exact duplicate; a repeat, 0 and 5000 are refused -- as is,
    under Normalized Cosine, every row at a distance above 0 from itself."""
    e = M.expected()[name]["remove"]
    src = M.make_index_dir(name, str(tmp_path / "in"))
    ix = base.Index(src)
    try:
        done = ix.batch_remove(e["ids"])
        assert [int(v) for v in done] == e["removed"]
        out = str(tmp_path / "out")
        ix.save(out)
        assert_removed_files(out, name, src)
        assert_answers_after_removal(ix, out, name)
    finally:
        ix.close()


def test_remove_one_call_per_id(tmp_path):
    name = "l1_u8_ties"
    e = M.expected()[name]["remove"]
    src = M.make_index_dir(name, str(tmp_path / "in"))
    ix = base.Index(src)
    try:
        done = []
        for i in e["ids"]:
            try:
                ix.remove(i)
                done.append(1)
            except NativeError:
                done.append(0)
        assert done == e["removed"]
        out = str(tmp_path / "out")
        ix.save(out)
        assert_removed_files(out, name, src)
    finally:
        ix.close()


def test_refine_after_remove_in_one_handle(tmp_path):
    """The removed rows are neither searched nor found; nothing is reopened in between."""
    name = M.REFINE_REMOVED_CASE
    e = M.expected()[name]["remove"]
    src = M.make_index_dir(name, str(tmp_path / "in"))
    ix = base.Index(src)
    try:
        assert [int(v) for v in ix.batch_remove(e["ids"])] == e["removed"]
        refine_anng(ix, M.REFINE_A[1])
        out = str(tmp_path / "out")
        ix.save(out)
    finally:
        ix.close()
    assert_grp(out, name, "refine_removed")
    assert_tre(out, name)
    assert M.sha256(read(out, "obj")) == e["obj_sha256"]
    assert_unchanged(out, src, ("prf",))


# ---- ONNG ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.ONNG_CASES)
def test_optimizer_execute(name, tmp_path):
    """Edge and path adjustment (-o 5 -i 20) of a graph whose lists are mostly ties."""
    src = M.make_index_dir(name, str(tmp_path / "in"))
    out = str(tmp_path / "out")
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    opt = L.ngt_create_optimizer(True, err)
    try:
        assert L.ngt_optimizer_set_minimum(opt, M.ONNG_OUTGOING, M.ONNG_INCOMING, -1, -1, err)
        assert L.ngt_optimizer_set_processing_modes(opt, False, False, False, err)
        assert L.ngt_optimizer_execute(opt, src.encode(), out.encode(), err), base._err_string(L, err)
    finally:
        L.ngt_destroy_optimizer(opt)
        L.ngt_destroy_error_object(err)
    assert_grp(out, name, "onng")
    assert F.read_prf(os.path.join(src, "prf"))["GraphType"] == "ANNG"
    assert F.read_prf(os.path.join(out, "prf"))["GraphType"] == M.expected()[name]["onng"]["graph_type"]
    assert_unchanged(out, src, ("obj", "tre"))
