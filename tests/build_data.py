"""Data of the construction cases (tests/golden/build_<case>/, build_cases.json).

The rows are not committed: they come from the seeded generators below, which
the fixture recipe (tests/golden/make_build_goldens.py) and the tests share.
Every case is one `ngt create -d <dim> -D <distance> -o <type> -b <batch>` of
its rows; build_index() is the same construction through the C API."""
import ctypes

import numpy as np

ROWS = 2000

# name -> `ngt create` -D letter, -o letter, dimension, -b.  l2_f4_onebatch's row
# count and batch size come from build_cases.json (one batch holds all its rows).
CASES = {
    "l2_f20": ("2", "f", 20, 200),
    "l1_u8_ties": ("1", "c", 8, 200),
    "l2_u8_ties": ("2", "c", 8, 2000),
    "ham_u8": ("h", "c", 16, 200),
    "jac_u8": ("j", "c", 16, 200),
    "cos_f100": ("c", "f", 100, 200),
    "ncos_f100": ("C", "f", 100, 200),
    "ang_u8": ("a", "c", 24, 200),
    "l1_f_dups": ("1", "f", 16, 200),
    "l2_f4_onebatch": ("2", "f", 4, None),
}
ONEBATCH_FIRST_ROWS = 30000  # grown by 5,000 until the reference tree has 300 internal nodes
ONEBATCH_STEP = 5000
ONEBATCH_MIN_INTERNAL = 300

DISTANCE_SETTER = {"1": "l1", "2": "l2", "h": "hamming", "j": "jaccard", "c": "cosine", "C": "normalized_cosine",
                   "a": "angle"}


def _ties_u8():
    """Rows over {0, 1, 2}: 3^8 = 6,561 possible rows give a few hundred exact
    duplicates among 2,000, and distances with few values.

    Uniform rows alone never leave a split short of five clusters: 101 of them
    are at ten or more different distances from any pivot.  So the first 101
    rows, which are the first leaf to split whatever the batch size, are the
    row of zeros, 64 of the 70 rows with four ones (all at L1 distance 4 and L2
    distance 2 from it, and close to one another), and the 36 rows that are all
    twos but for one or two ones (far from it, close to one another).  The row
    of zeros has by far the largest variance of distances, so it is the pivot,
    and with 64 of the 100 others at one distance the cluster walk ends at
    three clusters under either metric: FLT_MAX borders, and two leaves no
    object can reach.  The order of the 101 is shuffled."""
    rs = np.random.RandomState(21)
    rows = rs.randint(0, 3, (ROWS, 8))
    first = [np.zeros(8, dtype=rows.dtype)]
    for m in range(256):
        if bin(m).count("1") == 4:
            first.append(np.array([(m >> b) & 1 for b in range(8)], dtype=rows.dtype))
    first = first[:1] + [first[1 + i] for i in sorted(rs.permutation(70)[:64])]
    for i in range(8):
        for j in range(i, 8):
            p = np.full(8, 2, dtype=rows.dtype)
            p[i] = 1
            p[j] = 1
            first.append(p)
    assert len(first) == 101
    rows[:101] = np.array(first)[rs.permutation(101)]
    return rows


def _dups_f16():
    """30 % of the rows copy an earlier row -- alternately one of the same
    creation batch of 200 (where there is one) and one of any earlier row --
    and rows 900..1049 are one row 150 times, across the boundary at 1,000."""
    rs = np.random.RandomState(29)
    rows = rs.rand(ROWS, 16).astype(np.float32)
    copy = rs.rand(ROWS) < 0.3
    near = True
    for i in range(1, ROWS):
        if not copy[i]:
            continue
        start = i - i % 200
        src = rs.randint(start, i) if near and i > start else rs.randint(0, i)
        near = not near
        rows[i] = rows[src]
    rows[900:1050] = rows[900]
    return rows


def dataset(name, rows=None):
    """-> (rows as the CLI's text holds them, 'f' / 'c')."""
    otype = CASES[name][1]
    if name == "l2_f20":
        return np.random.RandomState(20).rand(ROWS, 20).astype(np.float32), otype
    if name in ("l1_u8_ties", "l2_u8_ties"):
        return _ties_u8(), otype
    if name == "ham_u8":
        return np.random.RandomState(22).randint(0, 256, (ROWS, 16)), otype
    if name == "jac_u8":
        r = np.random.RandomState(23).randint(0, 256, (ROWS, 16))
        r[~r.any(axis=1), 0] = 1  # Jaccard of two all-zero rows is 0 / 0
        return r, otype
    if name == "cos_f100":
        return (np.random.RandomState(24).rand(ROWS, 100) - 0.5).astype(np.float32), otype
    if name == "ncos_f100":
        return (np.random.RandomState(25).rand(ROWS, 100) - 0.5).astype(np.float32), otype
    if name == "ang_u8":
        return np.random.RandomState(26).randint(0, 256, (ROWS, 24)), otype
    if name == "l1_f_dups":
        return _dups_f16(), otype
    if name == "l2_f4_onebatch":
        # the first rows of one stream, so a larger n keeps the smaller one's rows
        return np.random.RandomState(27).rand(rows, 4).astype(np.float32), otype
    raise KeyError(name)


QUERIES = 32
STORED_QUERIES = 8  # the first queries of every case equal a stored row


def _queries(name):
    rows, otype = dataset(name)
    rs = np.random.RandomState(4000 + CASES[name][2] + len(name))
    pick = rs.permutation(ROWS)[:STORED_QUERIES]
    fresh = rows[rs.permutation(ROWS)[:QUERIES - STORED_QUERIES]]
    if otype == "f":
        fresh = (fresh * np.float32(1.01) + np.float32(0.003)).astype(np.float32)
    else:
        fresh = np.clip(fresh + rs.randint(-1, 2, fresh.shape), 0, 255)
    return np.concatenate([rows[pick], fresh]), pick


def queries(name):
    """The 32 search queries of a 2,000-row case (tests/golden/build_<case>/search.npz,
    make_search_matrix_goldens.py), as the CLI's text holds them: 8 stored rows,
    then 24 other rows perturbed -- scaled and shifted floats, uint8 values moved
    by -1, 0 or 1."""
    return _queries(name)[0]


def stored_query_rows(name):
    """The 0-based rows the first 8 queries equal."""
    return _queries(name)[1]


def write_text(rows, otype, path):
    """One object per line for `ngt create`: %.9g round-trips float32."""
    with open(path, "w") as f:
        for r in rows:
            f.write("\t".join(("%d" % v) if otype == "c" else ("%.9g" % v) for v in r) + "\n")


def create_args(name, batch):
    d, o, dim, _ = CASES[name]
    return ["create", "-d", str(dim), "-D", d, "-o", o, "-b", str(batch)]


# ---- the same construction through the C API ----------------------------------------
def open_index(path, name, batch):
    """ngt_create_graph_and_tree with the case's property (the CLI's defaults otherwise)
    -> (library, index handle, property handle, error handle)."""
    import ngt_amd
    from ngt_amd import base
    d, o, dim, _ = CASES[name]
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    prop = L.ngt_create_property(err)
    ok = L.ngt_set_property_dimension(prop, dim, err)
    ok = ok and getattr(L, "ngt_set_property_distance_type_" + DISTANCE_SETTER[d])(prop, err)
    ok = ok and (L.ngt_set_property_object_type_integer(prop, err) if o == "c"
                 else L.ngt_set_property_object_type_float(prop, err))
    ok = ok and L.ngt_set_property_edge_size_for_creation(prop, 10, err) and \
        L.ngt_set_property_edge_size_for_search(prop, 40, err)
    ok = ok and L.ngt_set_property_value(prop, b"BatchSizeForCreation", str(batch).encode(), err)
    ok = ok and L.ngt_set_property_value(prop, b"ThreadPoolSize", b"24", err)  # the CLI's default
    index = L.ngt_create_graph_and_tree(path.encode(), prop, err) if ok else None
    assert index, base._err_string(L, err)
    return L, index, prop, err


def append_and_create(L, index, err, rows):
    """ngt_batch_append_index of `rows`, then ngt_create_index."""
    from ngt_amd import base
    flat = np.ascontiguousarray(rows, dtype=np.float32)
    assert L.ngt_batch_append_index(index, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(flat), err), \
        base._err_string(L, err)
    assert L.ngt_create_index(index, 24, err), base._err_string(L, err)


def build_index(path, name, rows, batch, cuts=()):
    """The case built on the device and saved to `path`; `cuts` are row counts
    after which ngt_create_index runs before the next rows are appended."""
    from ngt_amd import base
    L, index, prop, err = open_index(path, name, batch)
    try:
        at = 0
        for end in list(cuts) + [len(rows)]:
            append_and_create(L, index, err, rows[at:end])
            at = end
        assert L.ngt_save_index(index, path.encode(), err), base._err_string(L, err)
    finally:
        L.ngt_close_index(index)
        L.ngt_destroy_property(prop)
        L.ngt_destroy_error_object(err)
    return path
