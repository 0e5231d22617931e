"""The search cases over the construction fixtures (tests/golden/build_<case>/):
the index the reference built, the 32 queries of build_data.queries() as the
oracle and the device see them, the reference's recorded results (search.npz,
make_search_matrix_goldens.py) and the oracle's, computed once per case and
shared by tests/test_search_matrix_host.py and tests/test_gpu_search_matrix.py."""
import ctypes
import functools
import os

import numpy as np

import build_data as D
import ngt_files as F
import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = [n for n in D.CASES if n != "l2_f4_onebatch"]
METRIC = {"1": "l1", "2": "l2", "h": "hamming", "j": "jaccard", "c": "cosine", "C": "normalized_cosine",
          "a": "angle"}
# tree-seeded modes of the fixture: key -> (k, epsilon); "t10w" and "t50w" are "t10r"
# and "t50" on an index opened read-write
TREE_MODES = {"t10r": (10, 0.1), "t10w": (10, 0.1), "t50": (50, 0.02), "t50w": (50, 0.02)}
READ_ONLY_MODES = ("t10r", "t50")
# linear modes: key -> (k, whether the fixture radius applies)
LINEAR_MODES = {"s10": (10, False), "s40r": (40, True)}
FLT_MAX = 3.402823466e38
# ncos_f100 against the reference: its query normalisation depends on the CPU model
# (DESIGN.md section 2), so a query whose oracle result list holds two adjacent
# distances within RTOL relative may be left out of an id comparison, at most
# NCOS_LEFT_OUT of the 32
RTOL = 1e-5
NCOS_LEFT_OUT = 2


class Case(object):
    pass


def prepared(metric, q, dim, dp, dtype):
    """One query as the index holds it while it searches: the object type's values,
    normalised for the normalized metrics (ObjectSpace::normalize restated in the
    reference's 16-lane order), zero-padded to the padded dimension."""
    out = np.zeros(dp, dtype)
    if dtype == np.uint8:
        out[:dim] = np.asarray(q).astype(np.int64).astype(np.uint8)
        return out
    v = np.array(q, dtype=np.float32)  # a copy: normalised in place
    if metric.startswith("normalized"):
        assert O.lib().ngto_normalize_f32(v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), dim) == 0
    out[:dim] = v
    return out


def read_only_metric(metric, otype):
    """The distance an index opened read-only walks its graph by
    (NeighborhoodGraph::Search::getMethod, Graph.h:290-317): the table has uint8
    entries for Hamming, Jaccard, L2 and L1 only and float entries for neither
    Hamming nor Jaccard, and every other combination is searched by L2 -- so
    `ngt search` (read-only unless -m w) ranks Angle or Cosine uint8 rows by L2
    and prints L2 distances.  The tree descent, linear search and an index
    opened read-write (the C API's ngt_open_index) use the index's comparator."""
    listed = ("hamming", "jaccard", "l2", "l1") if otype == "c" else (
        "normalized_cosine", "cosine", "normalized_angle", "angle", "normalized_l2", "l2", "l1", "sparse_jaccard",
        "poincare", "lorentz")
    return metric if metric in listed else "l2"


@functools.lru_cache(maxsize=None)
def load(name):
    d, o, dim, _ = D.CASES[name]
    c = Case()
    c.name, c.metric, c.otype, c.dim = name, METRIC[d], o, dim
    c.dtype = np.uint8 if o == "c" else np.float32
    c.dp = F.padded_dim(dim)
    gold = os.path.join(GOLD, "build_" + name)
    c.prop = F.read_prf(os.path.join(gold, "prf"))
    if name == "ncos_f100":
        # the rows the reference stored: it normalised them
        c.rows, _ = F.read_obj(os.path.join(gold, "obj"), dim, c.dtype)
    else:
        c.rows = np.zeros((D.ROWS + 1, c.dp), c.dtype)
        c.rows[1:, :dim] = D.dataset(name)[0]
    assert c.rows.shape == (D.ROWS + 1, c.dp)
    c.offs, c.ids, _ = F.read_grp(os.path.join(gold, "grp"))
    c.tree = F.read_tre(os.path.join(gold, "tre"), dim, c.dtype)
    c.seed_size = int(c.prop["SeedSize"])
    c.edge_size = int(c.prop["EdgeSizeForSearch"])
    c.queries = np.ascontiguousarray(D.queries(name), dtype=np.float32)
    c.stored = D.stored_query_rows(name)
    c.oq = np.stack([prepared(c.metric, q, dim, c.dp, c.dtype) for q in c.queries])
    path = os.path.join(gold, "search.npz")
    c.gold = dict(np.load(path)) if os.path.exists(path) else None
    c.radius = float(c.gold["radius"]) if c.gold else None
    # rows removed for the removal tests: 300 seeded ones and the rows the stored-row queries equal
    rs = np.random.RandomState(4100 + dim + len(name))
    c.valid = np.ones(D.ROWS + 1, np.uint8)
    c.valid[0] = 0
    c.valid[1 + rs.permutation(D.ROWS)[:300]] = 0
    c.valid[1 + c.stored] = 0
    return c


@functools.lru_cache(maxsize=None)
def oracle_tree(name, mode):
    """O.tree_seeds + O.search of the 32 queries -> [(ids, dists, counters, number of seeds)]."""
    c = load(name)
    k, eps = TREE_MODES[mode]
    walk = read_only_metric(c.metric, c.otype) if mode in READ_ONLY_MODES else c.metric
    out = []
    for q in c.oq:
        seeds, _, _ = O.tree_seeds(c.metric, c.tree, q, k, c.seed_size, c.dtype)
        ids, ds, cnt = O.search(walk, c.rows, c.offs, c.ids, q, seeds, k, np.float32(eps), edge_size=c.edge_size)
        out.append((ids, ds, cnt.copy(), len(seeds)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_linear(name, k, radius=-1.0, removed=False):
    """O.linear_search of the 32 queries -> [(ids, dists)]."""
    c = load(name)
    valid = c.valid if removed else None
    return [O.linear_search(c.metric, c.rows, q, k, valid=valid, radius=radius) for q in c.oq]


def fixture_radius(name):
    """The radius of the fixture's radius mode: the median over the queries of the
    oracle's 10th-nearest distance, as a float32."""
    tenth = [float(ds[9]) for _, ds in oracle_linear(name, 10)]
    return float(np.float32(np.median(np.array(tenth, np.float64))))


def has_ties(ds):
    return bool(np.any(ds[1:] == ds[:-1]))


def ascending_ids_within_ties(ids, ds):
    """Among equal distances the ids ascend (ObjectDistance::operator<, Common.h:1946-1959)."""
    same = ds[1:] == ds[:-1]
    return bool(np.all(ids[1:][same] > ids[:-1][same]))


def near_tie(ds):
    d = np.asarray(ds, np.float64)
    return bool(np.any(np.abs(d[1:] - d[:-1]) <= RTOL * np.abs(d[1:])))


def reference_ids(name, mode, i):
    gi = load(name).gold[mode + "_ids"][i]
    return gi[gi >= 0]


def assert_reference_ids(name, mode, results, first=0):
    """results: per query (ids, dists), query `first` onwards; the ids are the
    fixture's -> the queries left out (ncos_f100 only, near ties only)."""
    left_out = []
    for i, (ids, ds) in enumerate(results, first):
        if list(ids) == list(reference_ids(name, mode, i)):
            continue
        assert name == "ncos_f100" and near_tie(ds), (name, mode, i, list(ids), list(reference_ids(name, mode, i)))
        left_out.append(i)
    assert len(left_out) <= NCOS_LEFT_OUT, (name, mode, left_out)
    return left_out
