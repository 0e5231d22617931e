"""The removal fixtures of tests/golden/remove1k (make_remove_goldens.py)."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import ngt_files as F  # noqa: E402

RM = os.path.join(GOLD, "remove1k")
CASES = ["rm_one", "rm_seq", "rm_oneleaf", "rm_all", "rm_dup", "rm_onng"]


@functools.lru_cache(maxsize=None)
def expected():
    return json.load(open(os.path.join(RM, "expected.json")))


def input_files(name):
    """{file: path} of an input index; anng is refine1k's, onng shares its obj and tre."""
    anng = os.path.join(GOLD, "refine1k", "anng")
    if name == "anng":
        return {f: os.path.join(anng, f) for f in ("grp", "obj", "prf", "tre")}
    if name == "onng":
        return {"grp": os.path.join(RM, "onng", "grp"), "prf": os.path.join(RM, "onng", "prf"),
                "obj": os.path.join(anng, "obj"), "tre": os.path.join(anng, "tre")}
    return {f: os.path.join(RM, name, f) for f in ("grp", "obj", "prf", "tre")}


def copy_input(name, dst):
    import shutil
    os.makedirs(dst, exist_ok=True)
    for f, p in input_files(name).items():
        shutil.copy(p, os.path.join(dst, f))
    return dst


@functools.lru_cache(maxsize=None)
def load_input(name):
    """(rows, valid, offsets, ids, dists, tree, property) of an input index; shared, do not modify."""
    p = input_files(name)
    prop = F.read_prf(p["prf"])
    rows, valid = F.read_obj(p["obj"], 128, np.float32)
    offs, ids, dists = F.read_grp(p["grp"])
    tree = F.read_tre(p["tre"], 128, np.float32)
    for a in (rows, valid, offs, ids, dists):
        a.setflags(write=False)
    return rows, valid, offs, ids, dists, tree, prop


def leaf_lists(tree):
    lo = tree["leaf_off"]
    return [[int(v) for v in tree["leaf_ids"][int(lo[i]):int(lo[i + 1])]] for i in range(len(lo) - 1)]
