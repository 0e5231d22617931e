"""The construction fixtures (tests/golden/build_<case>/, made by the reference
CLI through make_build_goldens.py) hold what each is there for: conditions on
the reference's own output, read with ngt_files, so that a regenerated fixture
that lost its ties, duplicates or depth fails here instead of letting
tests/test_gpu_build_matrix.py pass for nothing."""
import json
import os

import numpy as np
import pytest

import build_data as D
import ngt_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_NGT = os.path.join(ROOT, "oracle", "_ref", "ngt")
CASES = json.load(open(os.path.join(GOLD, "build_cases.json")))
FLT_MAX = np.float32(3.4028234663852886e38)


def gold(name, f):
    return os.path.join(GOLD, "build_" + name, f)


def tree(name):
    _, o, dim, _ = D.CASES[name]
    return F.read_tre(gold(name, "tre"), dim, np.uint8 if o == "c" else np.float32)


def graph_nodes(name):
    offs, _, _ = F.read_grp(gold(name, "grp"))
    return int(np.count_nonzero(np.diff(offs.astype(np.int64))))


def test_every_case_has_its_files_and_parameters():
    assert set(CASES) == set(D.CASES)
    for name, (d, o, dim, batch) in D.CASES.items():
        entry = CASES[name]
        if name == "l2_f4_onebatch":
            assert entry["batch"] == entry["rows"] >= D.ONEBATCH_FIRST_ROWS
            assert (entry["rows"] - D.ONEBATCH_FIRST_ROWS) % D.ONEBATCH_STEP == 0
            assert len(entry["grp_sha256"]) == 64
            assert os.listdir(os.path.join(GOLD, "build_" + name)) == ["tre"]
            continue
        assert (entry["rows"], entry["batch"]) == (D.ROWS, batch)
        prop = F.read_prf(gold(name, "prf"))
        assert int(prop["Dimension"]) == dim and int(prop["BatchSizeForCreation"]) == batch
        assert prop["ObjectType"] == ("Integer-1" if o == "c" else "Float-4")
        offs, _, _ = F.read_grp(gold(name, "grp"))
        assert len(offs) - 1 == D.ROWS + 1
    for name in CASES:
        for f in os.listdir(os.path.join(GOLD, "build_" + name)):
            assert os.path.getsize(gold(name, f)) < 1000000, (name, f)


@pytest.mark.parametrize("name", ["l1_u8_ties", "l2_u8_ties"])
def test_tie_cases_hold_short_splits_and_empty_leaves(name):
    """Equal split distances left fewer than five clusters: an internal node with
    a FLT_MAX border, and the empty leaves behind it."""
    t = tree(name)
    valid = t["in_valid"].astype(bool)
    assert np.any(t["in_border"][valid] == FLT_MAX)
    counts = np.diff(t["leaf_off"].astype(np.int64))
    assert np.any((counts == 0) & t["leaf_valid"].astype(bool))


@pytest.mark.parametrize("name", ["l1_u8_ties", "l1_f_dups"])
def test_duplicate_cases_keep_objects_out_of_the_tree(name):
    """An object at distance 0 from its nearest neighbour gets a graph node and no leaf entry."""
    assert len(tree(name)["leaf_ids"]) < graph_nodes(name) == D.ROWS


def test_dups_case_has_an_edge_of_distance_zero():
    _, _, dists = F.read_grp(gold("l1_f_dups", "grp"))
    assert np.any(dists == 0.0)


def test_onebatch_case_is_deep_enough():
    t = tree("l2_f4_onebatch")
    assert int(t["in_valid"].sum()) >= D.ONEBATCH_MIN_INTERNAL
    assert len(t["leaf_ids"]) == CASES["l2_f4_onebatch"]["rows"]


def test_generators_are_what_the_cases_say():
    ties, _ = D.dataset("l1_u8_ties")
    assert np.array_equal(ties, D.dataset("l2_u8_ties")[0]) and set(np.unique(ties)) == {0, 1, 2}
    assert len(np.unique(ties, axis=0)) < len(ties)  # exact duplicates by birthday
    assert D.dataset("jac_u8")[0].any(axis=1).all()
    cos, _ = D.dataset("cos_f100")
    assert (cos < 0).any() and (cos > 0).any()
    dups, _ = D.dataset("l1_f_dups")
    first = {}
    within = across = 0
    for i, r in enumerate(dups):
        j = first.setdefault(r.tobytes(), i)
        if j != i:
            within += j // 200 == i // 200
            across += j // 200 != i // 200
    assert within + across >= 0.25 * len(dups) and within > 100 and across > 100
    assert (dups[900:1050] == dups[900]).all() and not (dups[1050] == dups[900]).all()
    a, _ = D.dataset("l2_f4_onebatch", 1000)
    b, _ = D.dataset("l2_f4_onebatch", 2000)
    assert np.array_equal(a, b[:1000])


@pytest.mark.skipif(not os.path.exists(REF_NGT), reason="the reference CLI (oracle/_ref/ngt) is not built")
@pytest.mark.parametrize("name", ["l1_u8_ties", "l1_f_dups", "l2_f20"])
def test_recipe_reproduces_the_small_fixtures(tmp_path, name):
    """The recipe's `ngt create` of three of the 2,000-row cases gives the committed
    files bit for bit (the whole recipe, the 50,000-row case included, takes minutes)."""
    import make_build_goldens as M
    src, entry, files = M.run_case(REF_NGT, name, str(tmp_path))
    assert entry == CASES[name]
    for f in files:
        assert open(os.path.join(src, f), "rb").read() == open(gold(name, f), "rb").read(), (name, f)
