"""The graph-type construction cases (tests/golden/gtype_<type>_<case>/).

Every case is 2,000 rows of a tests/build_data.py data set built by the
reference CLI with `ngt create -g k|i|o -E <edges> -S 40 -b 200`
(tests/golden/make_graph_type_goldens.py); build_index() is the same
construction through the C API.  KNNG is the reference run with one creation
thread (-p 1): with more its tre follows thread completion order.  IANNG and
ONNG run with the CLI's default 24 threads."""
import ctypes

import numpy as np

import build_data as D

BATCH = 200
GRAPH_TYPE_NAME = {"k": "KNNG", "i": "IANNG", "o": "ONNG"}
GRAPH_TYPE_ID = {"k": 2, "i": 5, "o": 4}


def _case(gtype, data, edges=10, out_in=(10, 80), cut=None, suffix=""):
    return {"gtype": gtype, "data": data, "edges": edges, "outgoing": out_in[0], "incoming": out_in[1],
            "cut": cut, "threads": 1 if gtype == "k" else 24,
            "dir": "gtype_%s_%s%s" % (GRAPH_TYPE_NAME[gtype].lower(), data, suffix)}


# cut: `ngt create` of the first `cut` rows, then `ngt append` of the rest
CASES = [
    _case("k", "l2_f20"),           # the tiled L2-float scan
    _case("k", "l1_u8_ties"),       # ties, and duplicates within the bound
    _case("k", "ham_u8"),
    _case("k", "cos_f100"),         # float, not L2
    _case("k", "l2_f20", edges=40, suffix="_e40"),       # k = 41
    _case("k", "l1_u8_ties", cut=1200, suffix="_inc"),
    _case("i", "l2_f20"),
    _case("i", "l1_u8_ties"),
    _case("i", "l1_f_dups"),
    _case("i", "ham_u8"),
    _case("o", "l2_f20"),
    _case("o", "l1_u8_ties"),
    _case("o", "l1_f_dups"),
    _case("o", "ham_u8"),
    _case("o", "l2_f20", out_in=(5, 30), suffix="_o5x30"),
    _case("o", "l2_f20", out_in=(20, 5), suffix="_o20x5"),  # outgoing above E, incoming below it
]
BY_DIR = {c["dir"]: c for c in CASES}


def create_args(case):
    """The `ngt create` arguments of a case (index and data file follow)."""
    args = D.create_args(case["data"], BATCH) + ["-E", str(case["edges"]), "-S", "40", "-g", case["gtype"],
                                                 "-p", str(case["threads"])]
    if case["gtype"] == "o" and (case["outgoing"], case["incoming"]) != (10, 80):
        args += ["-O", "%dx%d" % (case["outgoing"], case["incoming"])]
    return args


def dtype_of(case):
    return np.uint8 if D.CASES[case["data"]][1] == "c" else np.float32


# ---- the same construction through the C API ----------------------------------------
def set_graph_property(L, prop, err, case, batch=BATCH):
    ok = L.ngt_set_property_edge_size_for_creation(prop, case["edges"], err) and \
        L.ngt_set_property_edge_size_for_search(prop, 40, err)
    ok = ok and L.ngt_set_property_value(prop, b"BatchSizeForCreation", str(batch).encode(), err)
    ok = ok and L.ngt_set_property_value(prop, b"ThreadPoolSize", str(case["threads"]).encode(), err)
    ok = ok and L.ngt_set_property_value(prop, b"GraphType", GRAPH_TYPE_NAME[case["gtype"]].encode(), err)
    if case["gtype"] == "o":
        ok = ok and L.ngt_set_property_value(prop, b"OutgoingEdge", str(case["outgoing"]).encode(), err)
        ok = ok and L.ngt_set_property_value(prop, b"IncomingEdge", str(case["incoming"]).encode(), err)
    return ok


def new_property(L, err, data):
    """A property with the data set's dimension, metric and object type."""
    d, o, dim, _ = D.CASES[data]
    prop = L.ngt_create_property(err)
    ok = L.ngt_set_property_dimension(prop, dim, err)
    ok = ok and getattr(L, "ngt_set_property_distance_type_" + D.DISTANCE_SETTER[d])(prop, err)
    ok = ok and (L.ngt_set_property_object_type_integer(prop, err) if o == "c"
                 else L.ngt_set_property_object_type_float(prop, err))
    assert ok
    return prop


def build_index(path, case, rows, batch=BATCH, keep_open=False):
    """The case built on the device and saved to `path`: ngt_batch_append_index +
    ngt_create_index, once more after the cut of an incremental case, then
    ngt_save_index.  keep_open -> (library, live index handle, error handle)."""
    import ngt_amd
    from ngt_amd import base
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    prop = new_property(L, err, case["data"])
    index = None
    try:
        assert set_graph_property(L, prop, err, case, batch), base._err_string(L, err)
        index = L.ngt_create_graph_and_tree(path.encode(), prop, err)
        assert index, base._err_string(L, err)
        at = 0
        for end in ([case["cut"]] if case["cut"] else []) + [len(rows)]:
            flat = np.ascontiguousarray(rows[at:end], dtype=np.float32)
            assert L.ngt_batch_append_index(index, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(flat),
                                            err), base._err_string(L, err)
            assert L.ngt_create_index(index, case["threads"], err), base._err_string(L, err)
            at = end
        assert L.ngt_save_index(index, path.encode(), err), base._err_string(L, err)
        if keep_open:
            live, index = index, None
            return L, live, err
    finally:
        if index:
            L.ngt_close_index(index)
        L.ngt_destroy_property(prop)
        if not keep_open:
            L.ngt_destroy_error_object(err)
    return path
