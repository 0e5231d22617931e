"""The CPU restatement (oracle/) against the reference's `ngt search` on the nine
2,000-row construction cases (tests/golden/build_<case>/search.npz, made by
make_search_matrix_goldens.py): tree-seeded graph search and linear search under
L1, L2, Hamming, Jaccard, Cosine, Normalized Cosine and Angle, on float and
uint8 rows, with heavy distance ties and 30 % duplicate rows.  Ids and printed
distances are the reference's exactly, and so is the distance-computation count.

ncos_f100 is the one tolerance case: the reference normalises the query with
the CPU's reciprocal-square-root approximation, so its
distances are compared at 1e-5 relative, and a query whose oracle result list
holds two adjacent distances within 1e-5 relative may be left out of the id
comparison -- at most NCOS_LEFT_OUT of the 32.  The distance is 1 - q.x in float32,
and every query has a row it is (nearly) parallel to: there the difference
cancels to 0 .. 5e-05 and a relative bound says nothing (the oracle gives 0
where the reference gives 4.5e-08).  So the absolute 1e-6 of the comparator
tolerance cases of tests/test_gpu_parity.py, eight float32 steps of an inner
product near 1, is allowed on top."""
import os

import numpy as np
import pytest

import build_data as D
import search_matrix as S

REF_NGT = os.path.join(S.ROOT, "oracle", "_ref", "ngt")
NCOS_LEFT_OUT = S.NCOS_LEFT_OUT
RTOL = S.RTOL
ATOL = 1e-6


def fmt(x):
    # `stream << objects[i].distance` (Command.cpp:349): default 6 significant digits
    return "%g" % float(x)


def check_against_reference(name, mode, results):
    """results: per query (ids, dists) of the oracle; the fixture's mode holds the
    reference's.  -> the queries left out of the id comparison (ncos_f100 only)."""
    g = S.load(name).gold
    left_out = []
    for i, (ids, ds) in enumerate(results):
        gi = g[mode + "_ids"][i]
        gi = gi[gi >= 0]
        gd = g[mode + "_dists"][i][:len(gi)]
        if name != "ncos_f100":
            assert list(ids) == list(gi), (name, mode, i)
            assert [fmt(x) for x in ds] == [fmt(x) for x in gd], (name, mode, i)
            continue
        if list(ids) != list(gi):
            assert S.near_tie(ds), (name, mode, i)
            left_out.append(i)
            continue
        # six printed digits of the reference's value against the oracle's float
        np.testing.assert_allclose(ds.astype(np.float64), gd, rtol=RTOL, atol=ATOL, err_msg="%s %s %d" % (name, mode, i))
    assert len(left_out) <= NCOS_LEFT_OUT, (name, mode, left_out)
    return left_out


@pytest.mark.parametrize("mode", list(S.TREE_MODES))
@pytest.mark.parametrize("name", S.CASES)
def test_tree_seeded_search_matches_reference(name, mode):
    """`ngt search -i t` (GraphAndTreeIndex::search, Index.h:1570-1577)."""
    res = S.oracle_tree(name, mode)
    k = S.TREE_MODES[mode][0]
    assert all(len(ids) == k and not np.isnan(ds).any() for ids, ds, _, _ in res)
    left_out = check_against_reference(name, mode, [(ids, ds) for ids, ds, _, _ in res])
    if mode in ("t10w", "t50w"):
        # Graph.cpp:604 counts every evaluated neighbour; seeds are only
        # counted under NGT_DISTANCE_COMPUTATION_COUNT (Graph.cpp:287).
        g = S.load(name).gold
        for i, (_, _, cnt, nseeds) in enumerate(res):
            if i in left_out:
                continue
            assert int(cnt[0]) - nseeds == int(g[mode + "_ndist"][i]), (name, i)


@pytest.mark.parametrize("name", S.CASES)
def test_read_only_and_read_write_results(name):
    """The reference opened read-only returns what it returns read-write -- except on
    ang_u8, where its read-only table of distances has no Angle for uint8 rows
    and walks the graph by L2 (search_matrix.read_only_metric)."""
    g = S.load(name).gold
    same = all(np.array_equal(g[r + "_ids"], g[w + "_ids"]) and
               np.array_equal(g[r + "_dists"], g[w + "_dists"], equal_nan=True)
               for r, w in (("t10r", "t10w"), ("t50", "t50w")))
    assert same == (name != "ang_u8")
    if name == "ang_u8":
        assert S.read_only_metric("angle", "c") == "l2" and g["t10r_dists"].max() > 100 > g["t10w_dists"].max()


@pytest.mark.parametrize("mode", list(S.LINEAR_MODES))
@pytest.mark.parametrize("name", S.CASES)
def test_linear_search_matches_reference(name, mode):
    """`ngt search -i s` (ObjectSpaceRepository::linearSearch, ObjectSpaceRepository.h:466-502)."""
    k, with_radius = S.LINEAR_MODES[mode]
    c = S.load(name)
    res = S.oracle_linear(name, k, c.radius if with_radius else S.FLT_MAX)
    assert all(not np.isnan(ds).any() for _, ds in res)
    if not with_radius:
        assert all(len(ids) == k for ids, _ in res)
    check_against_reference(name, mode, res)


@pytest.mark.parametrize("name", S.CASES)
def test_tree_seed_counts(name):
    """The two tie cases have leaves shorter than SeedSize; everywhere else a leaf gives all 10 seeds."""
    n = [nseeds for _, _, _, nseeds in S.oracle_tree(name, "t10r")]
    if name.endswith("_u8_ties"):
        assert min(n) < 10 and max(n) == 10
    else:
        assert set(n) == {10}


@pytest.mark.parametrize("name", S.CASES)
def test_fixture_radius_is_the_recipe_and_does_not_degenerate(name):
    """The stored radius is the median 10th-nearest distance of the oracle, and it
    leaves at least 4 of the 32 queries short of 10 results and at least 4 with 10."""
    c = S.load(name)
    assert np.float32(c.radius) == np.float32(S.fixture_radius(name))
    n = [len(ids) for ids, _ in S.oracle_linear(name, 10, c.radius)]
    assert sum(x < 10 for x in n) >= 4 and sum(x == 10 for x in n) >= 4, n
    # the 40-result lists are the 10-result lists continued
    for (a, _), (b, _) in zip(S.oracle_linear(name, 10, c.radius), S.oracle_linear(name, 40, c.radius)):
        assert list(a) == list(b[:10])


@pytest.mark.parametrize("name,least", [("l1_u8_ties", 32), ("l2_u8_ties", 32), ("ham_u8", 32), ("l1_f_dups", 24),
                                        ("jac_u8", 16)])
def test_tie_cases_return_equal_distances(name, least):
    """What these cases are searched for: top-10 lists with equal adjacent distances,
    in the reference's own output, ordered by id within a run."""
    g = S.load(name).gold
    tied = 0
    for i in range(D.QUERIES):
        ids, ds = g["s10_ids"][i], g["s10_dists"][i]
        tied += S.has_ties(ds)
        assert S.ascending_ids_within_ties(ids, ds), (name, i)
    assert tied >= least, (name, tied)


def test_queries_are_the_recipe():
    for name in S.CASES:
        c = S.load(name)
        assert c.queries.shape == (D.QUERIES, c.dim) and len(c.stored) == D.STORED_QUERIES
        rows = D.dataset(name)[0]
        assert np.array_equal(c.queries[:D.STORED_QUERIES], rows[c.stored].astype(np.float32))
        if c.otype == "c":
            assert c.queries.min() >= 0 and c.queries.max() <= 255 and np.array_equal(c.queries, np.rint(c.queries))
        # a stored-row query has a row at distance 0 (Cosine and Angle: within rounding)
        if c.metric in ("l1", "l2", "hamming", "jaccard"):
            assert all(ds[0] == 0.0 for _, ds in S.oracle_linear(name, 10)[:D.STORED_QUERIES]), name


@pytest.mark.skipif(not os.path.exists(REF_NGT), reason="the reference CLI (oracle/_ref/ngt) is not built")
@pytest.mark.parametrize("name", ["l2_u8_ties", "l1_f_dups"])
def test_recipe_reproduces_the_fixture(tmp_path, name):
    """The recipe's rebuild and searches of two cases give the committed arrays bit for bit."""
    import make_search_matrix_goldens as M
    got = M.run_case(REF_NGT, name, str(tmp_path))
    want = S.load(name).gold
    assert set(got) == set(want)
    for key in want:
        a, b = np.asarray(got[key]), want[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, key)
