"""Data and checkers of the edge-count optimisation tests (ngt optimize-#-of-edges).

The data sets of tests/golden/edge_optimization.json are not committed: they
come from the seeded generators below, which the fixture recipe
(tests/golden/make_edge_optimization_goldens.py) and the tests share.

recut() restates GraphReconstructor::reconstructANNGFromANNG
(lib/NGT/GraphReconstructor.h:721-801) in numpy/Python; it is the checker of
ngt_amd_recut_anng."""
import ctypes

import numpy as np

ROWS = 25400      # two samples need 25,000 stored objects after 200 queries are drawn
SMALL_ROWS = 3000  # the refusals X1 / X2
DIM = 16


def f16():
    return np.random.RandomState(11).rand(ROWS, DIM).astype(np.float32)


def u8():
    return np.random.RandomState(12).randint(0, 256, (ROWS, DIM))


def dataset(name):
    """name: f16, u8 or u8_3000 -> (rows, object type 'f' / 'c')."""
    if name == "f16":
        return f16(), "f"
    if name == "u8":
        return u8(), "c"
    if name == "u8_3000":
        return u8()[:SMALL_ROWS], "c"
    raise KeyError(name)


def write_text(rows, otype, path):
    """One object per line for `ngt create`: %.9g round-trips float32."""
    with open(path, "w") as f:
        for r in rows:
            f.write("\t".join(("%d" % v) if otype == "c" else ("%.9g" % v) for v in r) + "\n")


def recut(offsets, ids, dists, K):
    """The re-cut of a CSR graph (slot 0 the dummy) to K edges.

    For id ascending, id's list is walked in order; an entry (m, d) with m < id
    goes to id's list as (m, d) and to m's list as (id, d), until K such entries
    were taken.  A distance below its predecessor's (the first one's predecessor
    is 0) ends the walk of that list.  Then every list is sorted by (distance,
    id) and an id equal to its predecessor's is dropped.  -0 comes back as +0, as
    from the device.  Returns (offsets, ids, dists)."""
    n = len(offsets) - 1
    lists = [[] for _ in range(n)]
    dists = np.asarray(dists, dtype=np.float32)
    for v in range(1, n):
        count = 0
        prev = np.float32(0.0)
        for e in range(int(offsets[v]), int(offsets[v + 1])):
            d = dists[e]
            if prev > d:
                break
            prev = d
            m = int(ids[e])
            if m < v:
                lists[v].append((d, m))
                lists[m].append((d, v))
                count += 1
            if count >= K:
                break
    out_off = np.zeros(n + 1, dtype=np.uint64)
    out_ids, out_d = [], []
    for v in range(1, n):
        # ObjectDistance::operator<: float comparison (-0 == +0), then the id
        lst = sorted(lists[v], key=lambda t: (float(t[0]), t[1]))
        prev = 0
        for d, m in lst:
            if m == prev:
                continue
            prev = m
            out_ids.append(m)
            out_d.append(d + np.float32(0.0))
        out_off[v + 1] = len(out_ids)
    return out_off, np.array(out_ids, dtype=np.uint32), np.array(out_d, dtype=np.float32)


# ---- the indexes and parameters of the cases, through the C API -----------------
def make_index(path, name):
    """The index `ngt create -d 16 -D 2 [-o c]` leaves, as far as the procedure
    reads it (prf and obj): the same objects appended through the C API and saved
    without a build."""
    import ngt_amd
    from ngt_amd import base
    rows, otype = dataset(name)
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    prop = L.ngt_create_property(err)
    ok = L.ngt_set_property_dimension(prop, DIM, err) and L.ngt_set_property_distance_type_l2(prop, err)
    ok = ok and L.ngt_set_property_edge_size_for_creation(prop, 10, err) and \
        L.ngt_set_property_edge_size_for_search(prop, 40, err)
    ok = ok and (L.ngt_set_property_object_type_integer(prop, err) if otype == "c"
                 else L.ngt_set_property_object_type_float(prop, err))
    ok = ok and L.ngt_set_property_value(prop, b"ThreadPoolSize", b"24", err)  # the CLI's default
    index = L.ngt_create_graph_and_tree(path.encode(), prop, err) if ok else None
    assert index, base._err_string(L, err)
    flat = np.ascontiguousarray(rows, dtype=np.float32)
    assert L.ngt_batch_append_index(index, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(flat), err), \
        base._err_string(L, err)
    assert L.ngt_save_index(index, path.encode(), err), base._err_string(L, err)
    L.ngt_close_index(index)
    L.ngt_destroy_property(prop)
    L.ngt_destroy_error_object(err)
    return path


def parameter(args):
    """NGTAnngEdgeOptimizationParameter of the CLI arguments of a case."""
    import ngt_amd
    p = ngt_amd.lib().ngt_get_anng_edge_optimization_parameter()
    opt = dict(zip(args[::2], args[1::2]))
    p.no_of_queries = int(opt.get("-q", p.no_of_queries))
    p.no_of_results = int(opt.get("-k", p.no_of_results))
    p.target_accuracy = float(opt.get("-a", p.target_accuracy))
    p.target_no_of_objects = int(opt.get("-o", p.target_no_of_objects))
    p.no_of_sample_objects = int(opt.get("-s", p.no_of_sample_objects))
    p.max_of_no_of_edges = int(opt.get("-e", p.max_of_no_of_edges))
    return p
