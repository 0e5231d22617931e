"""What each graph-type fixture (tests/golden/gtype_<type>_<case>/,
make_graph_type_goldens.py) has to contain, so that a mistake in the recipe
cannot hide behind a device build that repeats it."""
import os

import numpy as np
import pytest

import graph_type_data as G
import ngt_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ROWS = 2000
KNNG = [c for c in G.CASES if c["gtype"] == "k"]
ONNG = [c for c in G.CASES if c["gtype"] == "o"]


def graph(case):
    return F.read_grp(os.path.join(GOLD, case["dir"], "grp"))


def ids_of(case):
    return [c["dir"] for c in case]


def test_every_case_of_the_issue_is_present():
    assert len(G.CASES) == 16
    for c in G.CASES:
        for f in ("grp", "tre", "prf"):
            path = os.path.join(GOLD, c["dir"], f)
            assert os.path.getsize(path) < 1000000, path


@pytest.mark.parametrize("case", G.CASES, ids=ids_of(G.CASES))
def test_prf_names_the_type_and_the_edge_counts(case):
    prf = F.read_prf(os.path.join(GOLD, case["dir"], "prf"))
    assert prf["GraphType"] == G.GRAPH_TYPE_NAME[case["gtype"]]
    assert int(prf["EdgeSizeForCreation"]) == case["edges"]
    assert int(prf["OutgoingEdge"]) == case["outgoing"]
    assert int(prf["IncomingEdge"]) == case["incoming"]
    assert int(prf["BatchSizeForCreation"]) == G.BATCH and int(prf["EdgeSizeForSearch"]) == 40


@pytest.mark.parametrize("case", KNNG, ids=ids_of(KNNG))
def test_knng_nodes_hold_exactly_e_sorted_edges_and_no_self_edge(case):
    offs, ids, ds = graph(case)
    assert len(offs) == ROWS + 2
    for v in range(1, ROWS + 1):
        a, b = int(offs[v]), int(offs[v + 1])
        assert b - a == case["edges"], v
        assert v not in ids[a:b], v
        keys = list(zip(ds[a:b].tolist(), ids[a:b].tolist()))
        assert keys == sorted(keys), v


def test_incremental_knng_keeps_the_first_lists():
    case = G.BY_DIR["gtype_knng_l1_u8_ties_inc"]
    offs, ids, _ = graph(case)
    assert int(ids[int(offs[1]):int(offs[case["cut"] + 1])].max()) <= case["cut"]
    assert int(ids[int(offs[case["cut"] + 1]):].max()) > case["cut"]


def test_tie_case_has_a_tie_at_the_last_place():
    """Some list of l1_u8_ties ends at a distance that an object outside the
    list shares: there the id decided which of the two the list holds.  Without
    such a list the case would prove nothing about ties."""
    offs, ids, ds = graph(G.BY_DIR["gtype_knng_l1_u8_ties"])
    import build_data as D
    rows, _ = D.dataset("l1_u8_ties")
    tied = 0
    for v in range(1, ROWS + 1):
        a, b = int(offs[v]), int(offs[v + 1])
        last = ds[b - 1]
        d = np.abs(rows - rows[v - 1]).sum(axis=1).astype(np.float32)
        outside = np.ones(ROWS, bool)
        outside[ids[a:b] - 1] = False
        outside[v - 1] = False
        if np.any(d[outside] == last):
            tied += 1
    assert tied > 0


@pytest.mark.parametrize("case", ONNG, ids=ids_of(ONNG))
def test_onng_nodes_keep_at_least_the_outgoing_edges(case):
    offs, _, _ = graph(case)
    need = min(case["outgoing"], case["edges"])
    deg = np.diff(offs[1:ROWS + 2].astype(np.int64))
    assert len(deg) == ROWS and int(deg.min()) >= need
