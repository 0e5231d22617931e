"""The refine1k fixtures (tests/golden/make_refine_goldens.py) for the refine-anng tests."""
import functools
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
REFINE1K = os.path.join(GOLD, "refine1k")
sys.path.insert(0, GOLD)
import ngt_files as F  # noqa: E402

INT_MIN = -2 ** 31
# name -> (epsilon, expected accuracy, number of edges, explored edges, batch size, input fixture)
CASES = {
    "r_b256": (0.0, 0.0, 0, INT_MIN, 256, "anng"),
    "r_one": (0.0, 0.0, 0, INT_MIN, 10000, "anng"),
    "r_k10": (0.0, 0.0, 10, INT_MIN, 100, "anng"),
    "r_k30": (0.0, 0.0, 30, INT_MIN, 256, "anng"),
    "r_km30": (0.0, 0.0, -30, INT_MIN, 256, "anng"),
    "r_E10": (-0.1, 0.0, 0, 10, 256, "anng"),
    "r_a": (0.1, 0.8, 0, INT_MIN, 256, "anng_t"),
}


def make_index_dir(dst, src="anng"):
    """The input index directory `src` (anng, or anng_t with the accuracy table) at `dst`."""
    os.makedirs(dst)
    for f in ("grp", "obj", "tre"):
        shutil.copy(os.path.join(REFINE1K, "anng", f), os.path.join(dst, f))
    shutil.copy(os.path.join(REFINE1K, src, "prf"), os.path.join(dst, "prf"))
    return dst


@functools.lru_cache(maxsize=None)
def csr(name):
    """(offsets, ids, dists) of a fixture graph; shared, do not modify."""
    g = F.read_grp(os.path.join(REFINE1K, "anng" if name == "anng_t" else name, "grp"))
    for a in g:
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def index_parts():
    """(prop, rows, valid, tree) of the input index; shared, do not modify."""
    prop = F.read_prf(os.path.join(REFINE1K, "anng", "prf"))
    rows, valid = F.read_obj(os.path.join(REFINE1K, "anng", "obj"), 128, np.float32)
    tree = F.read_tre(os.path.join(REFINE1K, "anng", "tre"), 128, np.float32)
    return prop, rows, valid, tree
