"""CPU-side checks of refine-anng, object removal and the ONNG reconstruction
on the construction cases of tests/build_data.py: the obj writer that lets the
C API open the committed build_<case>/ directories, the plain-Python
restatements (refine_restate, remove_restate, onng_restate) against the files
the reference CLI wrote (tests/golden/stage_<case>/, stage_matrix.json), the
fixture recipe, and the conditions the fixtures exist for.  Ids and offsets are
compared exactly, distances as uint32 bits.  No device call is made here."""
import os
import tempfile

import numpy as np
import pytest

import build_data as D
import ngt_files as F
import onng_restate as ONNG
import oracle_py as O
import remove_restate as RM
import search_matrix as S
import stage_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_NGT = os.path.join(ROOT, "oracle", "_ref", "ngt")


def assert_same_graph(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "offsets")
    assert np.array_equal(got[1], want[1]), (what, "ids")
    assert np.array_equal(np.asarray(got[2], np.float32).view(np.uint32), want[2].view(np.uint32)), (what, "distances")


# ---- the obj writer ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", [(np.float32, 20), (np.uint8, 24), (np.float32, 16), (np.uint8, 16)])
def test_obj_round_trip(tmp_path, dtype, dim):
    rs = np.random.RandomState(7)
    dp = F.padded_dim(dim)
    rows = np.zeros((40, dp), dtype)
    rows[1:, :dim] = rs.randint(0, 256, (39, dim)) if dtype == np.uint8 else rs.randn(39, dim).astype(np.float32)
    valid = np.ones(40, np.uint8)
    valid[[0, 3, 39]] = 0
    path = str(tmp_path / "obj")
    F.write_obj(path, rows, dim, valid)
    assert os.path.getsize(path) == 8 + 40 + 37 * dim * np.dtype(dtype).itemsize
    got, gv = F.read_obj(path, dim, dtype)
    assert np.array_equal(gv, valid)
    assert got.dtype == rows.dtype and got[valid == 1].tobytes() == rows[valid == 1].tobytes()
    assert not got[valid == 0].any()
    # no mask: only the dummy slot is absent
    F.write_obj(path, rows, dim)
    assert list(np.flatnonzero(F.read_obj(path, dim, dtype)[1] == 0)) == [0]
    with pytest.raises(ValueError):
        F.obj_bytes(rows.astype(np.float64), dim)


def test_written_obj_equals_the_committed_one():
    assert M.obj_bytes("ncos_f100") == open(os.path.join(M.GOLD, "build_ncos_f100", "obj"), "rb").read()


@pytest.mark.parametrize("name", M.CASES)
def test_written_obj_has_the_reference_digest(name):
    """Before and after the removal: the reference's obj of the generated rows,
    and the same with '-' in the slots of the removed ones."""
    e = M.expected()[name]
    assert M.sha256(M.obj_bytes(name)) == e["obj_sha256"]
    assert M.sha256(M.obj_bytes(name, M.valid_after_removal(name))) == e["remove"]["obj_sha256"]


def test_assembled_directory_holds_the_committed_files(tmp_path):
    for name, stage in (("ham_u8", "build"), ("l1_f_dups", "remove")):
        c = S.load(name)
        d = M.make_index_dir(name, str(tmp_path / (name + stage)), stage)
        assert sorted(os.listdir(d)) == ["grp", "obj", "prf", "tre"]
        rows, valid = F.read_obj(os.path.join(d, "obj"), c.dim, c.dtype)
        assert rows.shape == c.rows.shape and int(valid.sum()) == \
            (D.ROWS if stage == "build" else D.ROWS - sum(M.expected()[name]["remove"]["removed"]))
        assert rows[valid == 1].tobytes() == c.rows[valid == 1].tobytes()
        assert M.sha256(os.path.join(d, "grp")) == (
            M.sha256(os.path.join(M.GOLD, "build_" + name, "grp")) if stage == "build"
            else M.expected()[name]["remove"]["grp_sha256"])


# ---- what is committed ----------------------------------------------------------------------
def test_every_case_has_its_files_and_digests():
    e = M.expected()
    assert sorted(e) == sorted(M.CASES)
    for name in M.CASES:
        assert sorted(k for k in e[name] if k != "obj_sha256") == sorted(M.stages_of(name))
        assert sorted(os.listdir(os.path.join(M.GOLD, "stage_" + name))) == sorted(M.stages_of(name))
        for stage in M.stages_of(name):
            d = os.path.join(M.GOLD, "stage_" + name, stage)
            assert [f[:3] for f in sorted(os.listdir(d))] == (["grp", "tre"] if stage == "remove" else ["grp"])
            for f in os.listdir(d):
                assert os.path.getsize(os.path.join(d, f)) < M.MAX_FILE, (name, stage, f)
            assert M.sha256(M.fixture_bytes(name, stage, "grp")) == e[name][stage]["grp_sha256"]
            assert M.sha256(M.fixture_bytes(name, stage, "grp")) != M.sha256(os.path.join(M.GOLD, "build_" + name, "grp"))
        assert M.sha256(M.fixture_bytes(name, "remove", "tre")) == e[name]["remove"]["tre_sha256"]
        assert e[name]["refine_a"]["args"] == M.REFINE_A[0]
    for name in M.REFINE_B_CASES:
        assert e[name]["refine_b"]["args"] == M.REFINE_B[0]
    for name in M.ONNG_CASES:
        assert e[name]["onng"]["args"] == M.ONNG_ARGS and e[name]["onng"]["graph_type"] == "ONNG"


# ---- the restatements against the reference's files ----------------------------------------
@pytest.mark.parametrize("name", M.CASES)
def test_refine_restatement_reproduces_refine_a(name):
    """Epsilon 0.1, eight batches, incoming edges.  On the tie and duplicate cases
    some refined list holds two neighbours at one distance, and some incoming edge
    goes into a list that holds its distance already."""
    stats = {}
    got = M.restate_refine(name, M.REFINE_A[1], M.graph(name, "build"), stats=stats)
    assert_same_graph(got, M.graph(name, "refine_a"), (name, "refine_a"))
    if name in M.TIE_CASES:
        assert M.has_list_with_equal_distances(M.graph(name, "refine_a"))
        assert stats.get("incoming_at_a_present_distance", 0) > 0


@pytest.mark.parametrize("name", M.REFINE_B_CASES)
def test_refine_restatement_reproduces_refine_b(name):
    """15 results per search, above EdgeSizeForCreation; no incoming edges; pruned to 15."""
    assert int(S.load(name).prop["EdgeSizeForCreation"]) < 15
    got = M.restate_refine(name, M.REFINE_B[1], M.graph(name, "build"))
    assert_same_graph(got, M.graph(name, "refine_b"), (name, "refine_b"))
    M.check_refine_b(name, M.graph(name, "refine_a"), M.graph(name, "refine_b"))


@pytest.mark.parametrize("name", M.CASES)
def test_remove_restatement_reproduces_the_removal(name):
    """Graph, outcomes, valid flags and each leaf's members in order.  The
    restatement keeps no leaf distances or leaf pivots, and ngt_files.read_tre
    parses none: those bytes of tre are compared on the device side only
    (tests/test_gpu_stage_matrix.py, byte for byte), here through the digest of
    the fixture alone."""
    c = S.load(name)
    e = M.expected()[name]["remove"]
    assert e["ids"] == M.removal_ids(name, c.offs, c.ids, c.tree, c.rows)
    M.check_removal(name, e, c.rows)
    valid = np.ones(D.ROWS + 1, np.uint8)
    valid[0] = 0
    offs, ids, dists = M.graph(name, "build")
    ix = RM.Index(c.metric, c.rows, valid, offs, ids, dists, c.tree, M.leaf_lists(c.tree), c.edge_size)
    done = [int(ix.remove(i)) for i in e["ids"]]
    assert done == e["removed"]
    assert_same_graph(ix.csr(), M.graph(name, "remove"), (name, "remove"))
    assert ix.leaves == M.leaf_lists(M.removed_tree(name))
    assert np.array_equal(ix.valid, M.valid_after_removal(name))
    # nothing but the leaves' members changed in the tree
    for key in ("in_pivot", "in_child", "in_border", "in_valid", "leaf_valid"):
        assert np.array_equal(M.removed_tree(name)[key], c.tree[key]), (name, key)
    assert M.removed_tree(name)["root"] == c.tree["root"]


def test_refine_restatement_reproduces_refine_after_remove():
    """The removed rows are not searched (isEmpty) and come back from no search."""
    name = M.REFINE_REMOVED_CASE
    valid = M.valid_after_removal(name)
    got = M.restate_refine(name, M.REFINE_A[1], M.graph(name, "remove"), tree=M.removed_tree(name), valid=valid)
    assert_same_graph(got, M.graph(name, "refine_removed"), (name, "refine_removed"))
    M.check_refine_removed(name, M.graph(name, "refine_removed"), valid)


@pytest.mark.parametrize("name", M.ONNG_CASES)
def test_onng_restatement_reproduces_onng(name):
    got = ONNG.reconstruct(*M.graph(name, "build"), M.ONNG_OUTGOING, M.ONNG_INCOMING, True, 0, input_is_anng=True)
    assert_same_graph(got, M.graph(name, "onng"), (name, "onng"))
    if name != "ham_u8":
        # the lists the two adjustments worked on are mostly ties
        offs, _, ds = M.graph(name, "build")
        o = offs.astype(np.int64)
        tied = sum(len(np.unique(ds[o[v]:o[v + 1]])) < o[v + 1] - o[v] for v in range(1, len(o) - 1))
        assert tied > D.ROWS // 2, (name, tied)


def test_fixtures_hold_queries_whose_leaf_was_emptied():
    """Four cases have a query that descends to the leaf their removal emptied."""
    hit = {}
    for name in M.CASES:
        c = S.load(name)
        hit[name] = [i for i, q in enumerate(c.oq)
                     if len(O.tree_seeds(c.metric, M.removed_tree(name), q, 10, c.seed_size, c.dtype)[0]) == 0]
    assert {n: h for n, h in hit.items() if h} == {"l2_f20": [29], "ham_u8": [23], "jac_u8": [0], "cos_f100": [12]}


# ---- the recipe -----------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(REF_NGT), reason="the reference CLI (oracle/_ref/ngt) is not built")
@pytest.mark.parametrize("name", M.CASES)
def test_recipe_reproduces_committed_fixtures(name):
    import make_stage_matrix_goldens as G
    with tempfile.TemporaryDirectory() as work:
        entry, dirs = G.run_case(REF_NGT, name, work)
        assert entry == M.expected()[name]
        for stage, f in G.committed_files(name):
            assert open(os.path.join(work, dirs[stage], f), "rb").read() == M.fixture_bytes(name, stage, f), (name, stage, f)
