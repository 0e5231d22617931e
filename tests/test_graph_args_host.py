"""What the graph stages refuse before they touch a device: the host checks of a
CSR argument and of each stage's own parameters in ngt_amd_onng_reconstruct,
ngt_amd_recut_anng, ngt_amd_refine_prune and ngt_amd_refine_merge, and the three
thread-local result slots while empty.  The messages are compared whole."""
import threading

import numpy as np
import pytest

import ngt_amd
from ngt_amd import edges, onng, refine

OFF = [0, 0, 1, 2]
IDS = np.array([2, 1], np.uint32)
DS = np.array([1, 1], np.float32)
RES = (np.array([[2]], np.uint32), np.array([[1]], np.float32), np.array([1], np.uint32))


def reconstruct(off, outgoing=1, incoming=1, device=0):
    return onng.reconstruct(off, IDS, DS, outgoing, incoming, False, device=device)


def recut(off, K=5):
    return edges.recut(off, IDS, DS, K)


def prune(off):
    return refine.prune(off, IDS, DS, 1)


def merge(off, first_id=1):
    return refine.merge(off, IDS, DS, first_id, RES[0], RES[1], RES[2], True)


STAGES = {"ngt_amd_onng_reconstruct": reconstruct, "ngt_amd_recut_anng": recut,
          "ngt_amd_refine_prune": prune, "ngt_amd_refine_merge": merge}
REFINE = ("ngt_amd_refine_prune", "ngt_amd_refine_merge")
NO_DEVICE = "%s: no HIP device available (the MI355X path has no CPU fallback)"


def refusal(call, *args, **kw):
    with pytest.raises(ngt_amd.NativeError) as e:
        call(*args, **kw)
    return str(e.value)


@pytest.mark.parametrize("who", sorted(STAGES))
def test_decreasing_offsets_name_the_node(who):
    assert refusal(STAGES[who], [0, 2, 1, 2]) == "%s: offsets decrease at node 1" % who


@pytest.mark.parametrize("who", sorted(STAGES))
def test_offsets_start_at_zero(who):
    assert refusal(STAGES[who], [1, 1, 2, 2]) == "%s: offsets[0] is not 0" % who


@pytest.mark.parametrize("who", REFINE)
def test_a_list_on_slot_zero_is_refused_by_refine(who):
    assert refusal(STAGES[who], [0, 1, 2, 2]) == "%s: slot 0 is the dummy and has no list" % who


def test_onng_parameters():
    assert refusal(reconstruct, OFF, outgoing=-1) == \
        "ngt_amd_onng_reconstruct: outgoing and incoming must not be negative"
    assert refusal(reconstruct, OFF, incoming=-1) == \
        "ngt_amd_onng_reconstruct: outgoing and incoming must not be negative"
    assert refusal(reconstruct, OFF, incoming=10001) == "ngt_amd_onng_reconstruct: something wrong. Edge size=10001"


def test_recut_parameters():
    assert refusal(recut, OFF, K=0) == "ngt_amd_recut_anng: K must be positive"


def test_merge_first_id():
    assert refusal(merge, OFF, first_id=3) == "ngt_amd_refine_merge: first id 3 outside [1, 3)"


# a graph that passes the host checks gets as far as the device; onng and recut take a list on slot 0
PASSING = [(who, OFF) for who in sorted(STAGES)] + [(who, [0, 1, 2, 2]) for who in sorted(STAGES) if who not in REFINE]


@pytest.mark.skipif(ngt_amd.device_count() > 0, reason="a device is present")
@pytest.mark.parametrize("who,off", PASSING)
def test_a_graph_that_passes_the_checks_without_a_device(who, off):
    assert refusal(STAGES[who], off) == NO_DEVICE % who


GETTERS = {"ngt_amd_onng_get_graph": "no reconstructed graph on this thread",
           "ngt_amd_recut_get_graph": "no re-cut graph on this thread",
           "ngt_amd_refine_get_graph": "no refined graph on this thread"}


@pytest.mark.parametrize("getter", sorted(GETTERS))
def test_getter_on_a_thread_with_no_run(getter):
    out = []

    def ask():
        L = ngt_amd.lib()
        off = np.zeros(4, np.uint64)
        out.append((getattr(L, getter)(off.ctypes.data, None, None), ngt_amd.last_error()))

    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert out == [(-1, "%s: %s" % (getter, GETTERS[getter]))]
