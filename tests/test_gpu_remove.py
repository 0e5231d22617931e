"""GPU: object removal (ngt_remove_index, ngt_batch_remove_index,
ngt_amd_remove_relink) against the reference-built fixtures of
tests/golden/remove1k and the plain-Python restatement (tests/remove_restate.py)."""
import ctypes
import filecmp
import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
import remove_data as D
import remove_restate as R
from ngt_amd import NativeError, base, ngtpy
from ngt_amd.device import DeviceIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = "Not in-memory or invalid offset of node. idx=%d size=%d"


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def assert_case_files(case, out):
    e = D.expected()[case]
    for f in ("grp", "tre"):
        assert filecmp.cmp(os.path.join(out, f), os.path.join(D.RM, case, f), shallow=False), (case, f)
    assert sha256(os.path.join(out, "obj")) == e["obj_sha256"]
    assert sha256(os.path.join(out, "prf")) == e["prf_sha256"]


# ---- the relink kernel ------------------------------------------------------------
def check_relink(ix, metric, rows, nbr):
    la, lb, ld = ix.remove_relink(nbr)
    want = R.relink_chain(metric, rows, nbr)
    assert len(la) == len(want) == max(len(nbr) - 1, 0)
    assert [int(v) for v in la] == [w[0] for w in want]
    assert [int(v) for v in lb] == [w[1] for w in want]
    assert np.array_equal(ld.view(np.uint32), np.array([w[2] for w in want], np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def dup_index():
    rows = D.load_input("dup")[0]
    ix = DeviceIndex("l2", "float", 128)
    ix.set_objects(rows)
    yield ix, rows
    ix.close()


def dup_lists(cap):
    """Lists over `dup`, whose rows 901..1000 repeat 1..100: equal distances
    occur before and after a swap."""
    rng = np.random.RandomState(7)
    pool = np.concatenate([np.arange(1, 101), np.arange(901, 1001), np.arange(300, 700)])
    return [rng.permutation(pool)[:d] for d in (1, 2, 3, 63, 64, 65, cap, cap + 1)]


def test_relink_l2_on_both_sides_of_the_capacity(dup_index):
    ix, rows = dup_index
    cap = DeviceIndex.remove_fast_path_capacity()
    assert 65 < cap < 400
    for nbr in dup_lists(cap):
        check_relink(ix, "l2", rows, nbr)
    check_relink(ix, "l2", rows, [5, 905, 17, 917, 5 + 900, 30])  # a row twice in one list


def test_relink_matrix_path_sees_the_same_lists(dup_index, monkeypatch):
    ix, rows = dup_index
    monkeypatch.setenv("NGT_AMD_REMOVE_FAST_CAP", "8")
    for nbr in dup_lists(DeviceIndex.remove_fast_path_capacity()):
        check_relink(ix, "l2", rows, nbr)


def test_relink_the_hub_of_the_fixture():
    rows, _, offs, ids, _, _, _ = D.load_input("anng")
    ix = DeviceIndex("l2", "float", 128)
    ix.set_objects(rows)
    nbr = ids[int(offs[17]):int(offs[18])]
    assert len(nbr) == 439
    check_relink(ix, "l2", rows, nbr)
    ix.close()


@pytest.mark.parametrize("metric,otype,dim", [("normalized_cosine", "float", 100), ("l1", "uint8", 100)])
def test_relink_other_metrics_and_padded_rows(metric, otype, dim, monkeypatch):
    rng = np.random.RandomState(3)
    n = 260
    dp = (dim + 15) // 16 * 16
    if otype == "float":
        rows = np.zeros((n, dp), np.float32)
        rows[1:, :dim] = rng.rand(n - 1, dim).astype(np.float32)
        for r in rows[1:]:
            O.lib().ngto_normalize_f32(r.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), dim)
    else:
        rows = np.zeros((n, dp), np.uint8)
        rows[1:, :dim] = rng.randint(0, 256, (n - 1, dim))
    rows[200:230] = rows[1:31]  # repeated rows: ties
    ix = DeviceIndex(metric, otype, dim)
    ix.set_objects(rows)
    cap = DeviceIndex.remove_fast_path_capacity()
    lists = [rng.permutation(np.arange(1, n))[:d] for d in (3, 65, cap, cap + 1)]
    for nbr in lists:
        check_relink(ix, metric, rows, nbr)
    monkeypatch.setenv("NGT_AMD_REMOVE_FAST_CAP", "8")
    check_relink(ix, metric, rows, lists[1])
    ix.close()


# ---- the six cases through the C API ------------------------------------------------
@pytest.mark.parametrize("case", D.CASES)
def test_batch_remove_writes_the_reference_files(case, tmp_path):
    e = D.expected()[case]
    ix = base.Index(D.copy_input(e["input"], str(tmp_path / "in")))
    done = ix.batch_remove(e["ids"])
    assert [int(v) for v in done] == e["removed"]
    out = str(tmp_path / "out")
    ix.save(out)
    ix.close()
    assert_case_files(case, out)


def test_remove_index_one_call_per_id(tmp_path):
    e = D.expected()["rm_seq"]
    ix = base.Index(D.copy_input("anng", str(tmp_path / "in")))
    size = int(ix._L.ngt_get_object_repository_size(ix.index, ix.err))
    for i, ok in zip(e["ids"], e["removed"]):
        if ok:
            ix.remove(i)
            continue
        before = str(tmp_path / ("before%d" % i))
        ix.save(before)
        assert not ix._L.ngt_remove_index(ix.index, i, ix.err)
        msg = base._err_string(ix._L, ix.err)
        assert msg.startswith("Capi : ngt_remove_index() : Error: ") and MISSING % (i, size) in msg, msg
        after = str(tmp_path / ("after%d" % i))
        ix.save(after)
        for f in ("grp", "tre", "obj", "prf"):
            assert filecmp.cmp(os.path.join(before, f), os.path.join(after, f), shallow=False), (i, f)
    out = str(tmp_path / "out")
    ix.save(out)
    ix.close()
    assert_case_files("rm_seq", out)


def same_as_linear(ix, queries, k, gone):
    gi, gd, gn = ix.batch_search(queries, k=k, epsilon=1.0)
    li, ld, ln = ix.batch_linear_search(queries, k=k)
    assert np.array_equal(gn, ln) and np.array_equal(gi, li)
    assert np.array_equal(gd.view(np.uint32), ld.view(np.uint32))
    assert not (set(gi.ravel().tolist()) & set(gone))
    return gi


def test_live_handle_after_rm_dup(tmp_path):
    e = D.expected()["rm_dup"]
    rows = D.load_input("dup")[0]
    ix = base.Index(D.copy_input("dup", str(tmp_path / "in")))
    size = int(ix._L.ngt_get_object_repository_size(ix.index, ix.err))
    ix.batch_search(rows[1:3, :128], k=5)  # the device copy exists before the removal
    assert ix.batch_remove(e["ids"]).all()
    # the removed rows themselves as queries, and others
    q = np.concatenate([rows[e["ids"], :128], rows[101:146, :128]])
    assert len(q) == 50
    same_as_linear(ix, q, 10, e["ids"])
    for i in e["ids"]:
        with pytest.raises(NativeError, match=" %d:%d" % (i, size)):
            ix.get_object(i)
        with pytest.raises(NativeError, match="idx=%d" % i):
            ix.get_edges(i)
    assert int(ix._L.ngt_get_object_repository_size(ix.index, ix.err)) == size
    ix.close()


def test_emptied_subtree_stays_valid(tmp_path):
    """The reference collapses an internal node whose five children are all
    empty leaves (Tree.cpp:338-397) and corrupts this index doing so; here the
    emptied leaves stay, and the saved index serves every remaining object."""
    rows, _, _, _, _, tree, _ = D.load_input("anng")
    child = tree["in_child"][6]
    assert all(c & 0x80000000 for c in child)
    leaves = D.leaf_lists(tree)
    gone = sorted(i for c in child for i in leaves[int(c) & 0x7FFFFFFF])
    assert len(gone) == 171
    ix = base.Index(D.copy_input("anng", str(tmp_path / "in")))
    assert ix.batch_remove(gone).all()
    out = str(tmp_path / "out")
    ix.save(out)
    ix.close()
    after = D.F.read_tre(os.path.join(out, "tre"), 128, np.float32)
    assert [len(D.leaf_lists(after)[int(c) & 0x7FFFFFFF]) for c in child] == [0] * 5
    ix = base.Index(out)
    left = np.array([i for i in range(1, 1001) if i not in set(gone)])
    gi = same_as_linear(ix, rows[left, :128], 5, gone)
    assert np.array_equal(gi[:, 0], left)
    ix.close()


def test_remove_then_insert_build_save_reload(tmp_path):
    rows = D.load_input("anng")[0]
    gone = [500, 17, 3, 999, 1000]
    ix = base.Index(D.copy_input("anng", str(tmp_path / "in")))
    assert ix.batch_remove(gone).all()
    new = (rows[gone + [20, 21, 22, 23, 24], :128] + np.float32(0.25)).astype(np.float32)
    ids = [ix.insert_object(r) for r in new[:5]]
    ix.batch_append(new[5:])
    assert ids == list(range(1001, 1006))
    ix.build_index()
    out = str(tmp_path / "out")
    ix.save(out)
    ix.close()
    ix = base.Index(out)
    gi = same_as_linear(ix, new, 5, gone)
    assert np.array_equal(gi[:, 0], np.arange(1001, 1011))
    same_as_linear(ix, rows[gone, :128], 5, gone)
    ix.close()


def test_ngtpy_remove_zero_based(tmp_path):
    rows = D.load_input("anng")[0]
    ix = ngtpy.Index(D.copy_input("anng", str(tmp_path / "in")))
    ix.remove(499)  # object 500
    with pytest.raises(NativeError, match="idx=500 size=1001"):
        ix.remove(499)
    assert 499 not in [int(r[0]) for r in ix.search(rows[500, :128], size=10, epsilon=0.3)]
    ix.save()
    ix.close()
    assert_case_files("rm_one", str(tmp_path / "in"))


@pytest.mark.parametrize("mode", [[], ["one"]])
def test_cxx_remove_sample_writes_rm_seq(mode, tmp_path):
    exe = str(tmp_path / "remove_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "remove_sample.cpp"),
                           "-L", os.path.join(ROOT, "ngt_amd"), "-lngt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "ngt_amd")])
    e = D.expected()["rm_seq"]
    idx = D.copy_input("anng", str(tmp_path / "in"))
    with open(str(tmp_path / "ids"), "w") as f:
        f.write("".join("%d\n" % i for i in e["ids"]))
    r = subprocess.run([exe, idx, str(tmp_path / "ids")] + mode, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if mode:
        assert [int(l.split()[1]) for l in r.stdout.splitlines() if l.startswith("refused ")] == [17, 0, 5000]
    assert_case_files("rm_seq", idx)
