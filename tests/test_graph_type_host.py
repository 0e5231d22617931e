"""Host side of graph-type construction through libngt_amd.so: the property's
GraphType, OutgoingEdge and IncomingEdge, and the refusals ngt_create_index
makes before any device work.  No GPU is needed."""
import ctypes

import pytest

import ngt_amd
from ngt_amd import base


def get_value(L, prop, err, key):
    buf = ctypes.create_string_buffer(64)
    assert L.ngt_get_property_value(prop, key, buf, 64, err) >= 0, base._err_string(L, err)
    return buf.value.decode()


@pytest.fixture
def env():
    L = ngt_amd.lib()
    err = L.ngt_create_error_object()
    prop = L.ngt_create_property(err)
    assert L.ngt_set_property_dimension(prop, 8, err)
    yield L, prop, err
    L.ngt_destroy_property(prop)
    L.ngt_destroy_error_object(err)


@pytest.mark.parametrize("gtype", ["KNNG", "IANNG", "ONNG"])
def test_graph_type_and_edge_counts_survive_set_get_save_open(env, tmp_path, gtype):
    L, prop, err = env
    want = {"GraphType": gtype, "OutgoingEdge": "7", "IncomingEdge": "33"}
    for k, v in want.items():
        assert L.ngt_set_property_value(prop, k.encode(), v.encode(), err)
    for k, v in want.items():
        assert get_value(L, prop, err, k.encode()) == v
    path = str(tmp_path / gtype).encode()
    index = L.ngt_create_graph_and_tree(path, prop, err)
    assert index, base._err_string(L, err)
    assert L.ngt_save_index(index, path, err), base._err_string(L, err)
    L.ngt_close_index(index)
    index = L.ngt_open_index(path, err)
    assert index, base._err_string(L, err)
    got = L.ngt_create_property(err)
    try:
        assert L.ngt_get_property(index, got, err)
        for k, v in want.items():
            assert get_value(L, got, err, k.encode()) == v
    finally:
        L.ngt_destroy_property(got)
        L.ngt_close_index(index)
    with open(tmp_path / gtype / "prf") as f:
        prf = dict(line.rstrip("\n").split("\t", 1) for line in f if "\t" in line)
    for k, v in want.items():
        assert prf[k] == v


def test_edge_counts_default_to_the_reference_values(env):
    L, prop, err = env
    assert get_value(L, prop, err, b"GraphType") == "ANNG"
    assert get_value(L, prop, err, b"OutgoingEdge") == "10"
    assert get_value(L, prop, err, b"IncomingEdge") == "80"
    assert get_value(L, prop, err, b"IncrimentalEdgeSizeLimitForTruncation") == "0"


def create_index_error(L, prop, err):
    index = L.ngt_create_graph_and_tree_in_memory(prop, err)
    assert index, base._err_string(L, err)
    try:
        row = (ctypes.c_float * 16)(*range(16))
        assert L.ngt_batch_append_index(index, ctypes.cast(row, ctypes.POINTER(ctypes.c_float)), 2, err)
        assert not L.ngt_create_index(index, 4, err)
        return L.ngt_get_error_string(err).decode()
    finally:
        L.ngt_close_index(index)


@pytest.mark.parametrize("gtype", ["BKNNG", "DNNG"])
def test_unsupported_graph_types_are_refused_by_name(env, gtype):
    L, prop, err = env
    assert L.ngt_set_property_value(prop, b"GraphType", gtype.encode(), err)
    msg = create_index_error(L, prop, err)
    assert msg == "Capi : ngt_create_index() : Error: index construction supports graphType ANNG, KNNG, IANNG and " \
                  "ONNG only"


def test_onng_with_truncation_is_refused_with_the_reference_text(env):
    L, prop, err = env
    assert L.ngt_set_property_value(prop, b"GraphType", b"ONNG", err)
    assert L.ngt_set_property_value(prop, b"IncrimentalEdgeSizeLimitForTruncation", b"7", err)
    msg = create_index_error(L, prop, err)
    assert "NGT::insertONNGNode: truncation should be disabled!" in msg
