"""Tree-seeded graph search and linear search on the device across the
construction cases of tests/build_data.py: L1, L2, Hamming, Jaccard, Cosine,
Normalized Cosine and Angle, float and uint8 rows, heavy distance ties and 30 %
duplicate rows, on the indexes the reference built (tests/golden/build_<case>/).

Every table has 2,001 rows.  The device is compared bit for bit with the CPU
restatement (tests/search_matrix.py computes it once per case), which
tests/test_search_matrix_host.py pins to the reference's `ngt search`, and its
ids with the reference's recorded results (search.npz; ncos_f100 under the
rule of search_matrix.assert_reference_ids).

The linear searches reach ngt_linear_search_kernel -- the scan of every metric
but L2 / Cosine float, of every uint8 index, of fewer than 32 queries and of k
above 32 -- through 64-row chunks, lists longer than a chunk, slices shorter
than k (~0 padding in the merge), k above the row count, a finite radius,
radius 0 and removed rows."""
import os

import numpy as np
import pytest

import build_data as D
import oracle_py as O
import search_matrix as S
from ngt_amd import NativeError, base
from ngt_amd.device import SEED_TREE, DeviceIndex

pytestmark = pytest.mark.gpu

# all the queries in one call, fewer than 32 (no batched scan takes them), one alone
BATCHES = [slice(0, 32), slice(0, 5), slice(0, 1)]
_INDEXES = {}


def device_index(name, removed=False):
    if (name, removed) not in _INDEXES:
        c = S.load(name)
        ix = DeviceIndex(c.metric, "float" if c.otype == "f" else "uint8", c.dim)
        ix.set_objects(c.rows, c.valid if removed else None)
        ix.set_graph(c.offs, c.ids)
        ix.set_tree(c.tree)
        ix.set_search_property(int(c.prop["EdgeSizeForSearch"]), int(c.prop["DynamicEdgeSizeBase"]),
                               int(c.prop["DynamicEdgeSizeRate"]), int(c.prop["SeedSize"]), 0)
        _INDEXES[(name, removed)] = ix
    return _INDEXES[(name, removed)]


@pytest.fixture(scope="module", autouse=True)
def close_indexes():
    yield
    for ix in _INDEXES.values():
        ix.close()
    _INDEXES.clear()


def assert_lists_equal(got, want, what):
    """got: (ids [nq, k], dists [nq, k], n [nq]) of the device; want: per query (ids, dists) of the oracle."""
    gi, gd, gn = got
    assert len(gn) == len(want), what
    for i, (oid, od) in enumerate(want):
        assert int(gn[i]) == len(oid), what + (i, int(gn[i]), len(oid))
        assert list(gi[i, :gn[i]]) == list(oid), what + (i,)
        assert np.array_equal(gd[i, :gn[i]].view(np.uint32), od.view(np.uint32)), what + (i,)
        assert S.ascending_ids_within_ties(gi[i, :gn[i]], gd[i, :gn[i]]), what + (i,)


def device_lists(got):
    gi, gd, gn = got
    return [(gi[i, :gn[i]], gd[i, :gn[i]]) for i in range(len(gn))]


# ---------------------------------------------------------------------------
# tree-seeded search
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["t10w", "t50w"])
@pytest.mark.parametrize("name", S.CASES)
def test_tree_seeded_search(name, mode):
    """ngt_tree_seed_kernel + graph search under every metric of the matrix, the
    queries mostly not stored rows: ids, distance bits and the number of
    distances computed equal the oracle's, the ids the reference's.  (The
    fixture's read-write modes: the reference opened read-only walks ang_u8 by
    L2, search_matrix.read_only_metric; everywhere else both modes hold the
    same results, tests/test_search_matrix_host.py.)"""
    c = S.load(name)
    k, eps = S.TREE_MODES[mode]
    ix = device_index(name)
    assert ix.resolve_edge_size(-1, eps) == c.edge_size
    gi, gd, gn, cnt = ix.search(c.queries, k=k, epsilon=eps, seed_mode=SEED_TREE)
    want = S.oracle_tree(name, mode)
    assert_lists_equal((gi, gd, gn), [(ids, ds) for ids, ds, _, _ in want], (name, mode))
    for i, (_, _, ocnt, _) in enumerate(want):
        assert int(cnt[i, 0]) == int(ocnt[0]), (name, mode, i)
    S.assert_reference_ids(name, mode, device_lists((gi, gd, gn)))


# ---------------------------------------------------------------------------
# linear search
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 33, 100, 300, 2100])
@pytest.mark.parametrize("name", S.CASES)
def test_linear_search(name, k):
    """k = 33 is past both batched scans' limits, 100 shifts the list across
    64-entry chunks, 300 is more than a slice holds (the merge reads ~0
    padding), 2,100 more than the table: every live row comes back."""
    c = S.load(name)
    ix = device_index(name)
    want = S.oracle_linear(name, k)
    assert all(len(ids) == min(k, D.ROWS) for ids, _ in want)
    for b in BATCHES:
        got = ix.linear_search(c.queries[b], k=k)
        assert_lists_equal(got, want[b], (name, k, b.stop))
        if k == 10:
            S.assert_reference_ids(name, "s10", device_lists(got))


@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("name", S.CASES)
def test_linear_search_within_a_radius(name, k):
    """The fixture radius leaves some queries short of 10 results and fills others;
    radius 0 returns the exact matches alone -- on the tie and duplicate cases
    several rows, in id order."""
    c = S.load(name)
    ix = device_index(name)
    for radius in (c.radius, 0.0):
        want = S.oracle_linear(name, k, radius)
        for b in BATCHES:
            got = ix.linear_search(c.queries[b], k=k, radius=radius)
            assert_lists_equal(got, want[b], (name, k, radius, b.stop))
            if radius == 0.0:
                assert all((ds == 0.0).all() for _, ds in device_lists(got))
            elif k == 40:
                S.assert_reference_ids(name, "s40r", device_lists(got))
    n = [len(ids) for ids, _ in S.oracle_linear(name, 10, c.radius)]
    assert sum(x < 10 for x in n) >= 4 and sum(x == 10 for x in n) >= 4, (name, n)
    if name in ("l1_u8_ties", "l2_u8_ties", "l1_f_dups"):
        assert max(len(ids) for ids, _ in S.oracle_linear(name, k, 0.0)) > 1, name


@pytest.mark.parametrize("with_radius", [False, True])
@pytest.mark.parametrize("name", S.CASES)
def test_linear_search_skips_removed_rows(name, with_radius):
    """300 seeded rows removed, and the row each stored-row query equals: none of
    them comes back, and k above the table returns the live rows."""
    c = S.load(name)
    ix = device_index(name, removed=True)
    live = int(c.valid.sum())
    assert live <= D.ROWS - 300 and not c.valid[1 + c.stored].any()
    radius = c.radius if with_radius else -1.0
    for k in (10, 300, 2100):
        want = S.oracle_linear(name, k, radius, True)
        if not with_radius:
            assert all(len(ids) == min(k, live) for ids, _ in want)
        for b in BATCHES[:2]:
            got = ix.linear_search(c.queries[b], k=k, radius=radius)
            assert_lists_equal(got, want[b], (name, k, with_radius, b.stop))
            assert all(c.valid[ids].all() for ids, _ in device_lists(got))


# ---------------------------------------------------------------------------
# k above the table, and above what the k-list's LDS holds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l2_f20", "ham_u8"])
def test_k_9000_returns_every_row(name):
    """The list a search keeps is never longer than the table, so k = 9,000 on
    2,001 rows is the search at k = 2,000: every row, nearest first."""
    c = S.load(name)
    ix = device_index(name)
    want = S.oracle_linear(name, 9000)
    assert all(len(ids) == D.ROWS for ids, _ in want)
    for b in BATCHES[:2]:
        assert_lists_equal(ix.linear_search(c.queries[b], k=9000), want[b], (name, b.stop))


def test_k_past_the_lds_limit_is_refused():
    """8,300 rows of 16 floats: the k-list, the chunk and the query fit the 65,536
    bytes a launch gets up to k = 8,119 (8 * 8,120 + 512 + 64), which returns
    the oracle's lists; k = 8,120 and 8,300 are refused before any launch."""
    rs = np.random.RandomState(4200)
    rows = np.zeros((8301, 16), np.float32)
    rows[1:, :4] = rs.rand(8300, 4).astype(np.float32)
    qs = rs.rand(2, 4).astype(np.float32)
    ix = DeviceIndex("l2", "float", 4)
    try:
        ix.set_objects(rows)
        gi, gd, gn = ix.linear_search(qs, k=8119)
        for i in range(2):
            q = np.zeros(16, np.float32)
            q[:4] = qs[i]
            oid, od = O.linear_search("l2", rows, q, 8119)
            assert int(gn[i]) == 8119 and list(gi[i]) == list(oid)
            assert np.array_equal(gd[i].view(np.uint32), od.view(np.uint32))
        for k in (8120, 8300):
            with pytest.raises(NativeError, match="LDS"):
                ix.linear_search(qs, k=k)
        gi, gd, gn = ix.linear_search(qs, k=10)  # the index still answers
        assert list(gn) == [10, 10] and list(gi[0]) == list(O.linear_search("l2", rows, np.pad(qs[0], (0, 12)), 10)[0])
    finally:
        ix.close()


# ---------------------------------------------------------------------------
# the C API on the one case with a committed obj
# ---------------------------------------------------------------------------
def test_capi_on_normalized_cosine():
    """ngt_search_index / ngt_linear_search_index on build_ncos_f100: one query per
    call, so the single-query path of the generic kernel under Normalized Cosine."""
    name = "ncos_f100"
    c = S.load(name)
    ix = base.Index(os.path.join(S.GOLD, "build_" + name))
    try:
        lo, hi = D.STORED_QUERIES - 4, D.STORED_QUERIES + 4  # four stored rows, four perturbed ones
        graph, linear = [], []
        for q in c.queries[lo:hi]:
            r = ix.search(q.astype(np.float64), 10, 0.1)
            graph.append((np.array([x.id for x in r]), np.array([x.distance for x in r], np.float32)))
            r = ix.linear_search(q.astype(np.float64), 10)
            linear.append((np.array([x.id for x in r]), np.array([x.distance for x in r], np.float32)))
        assert all(len(ids) == 10 for ids, _ in graph + linear)
        S.assert_reference_ids(name, "t10w", graph, first=lo)
        S.assert_reference_ids(name, "s10", linear, first=lo)
    finally:
        ix.close()
