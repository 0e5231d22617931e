"""The stages that run after construction -- refine-anng, object removal and
the ONNG reconstruction -- on the nine 2,000-row cases of tests/build_data.py:
the fixtures the reference CLI wrote (tests/golden/stage_<case>/ and
stage_matrix.json, make_stage_matrix_goldens.py), each case's input index
directory assembled from the committed build_<case>/ files plus a written obj,
the rule the removed ids follow, and the conditions the fixtures have to meet.
Shared by the recipe, tests/test_stage_matrix_host.py and
tests/test_gpu_stage_matrix.py."""
import functools
import gzip
import hashlib
import json
import os
import shutil

import numpy as np

import build_data as D
import ngt_files as F
import search_matrix as S

GOLD = S.GOLD
CASES = S.CASES
TIE_CASES = ("l1_u8_ties", "l2_u8_ties", "l1_f_dups")
INT_MIN = -2 ** 31
MAX_FILE = 1000000
GZIP_FROM = 900000  # a grp of this many bytes or more is committed as grp.gz

# stage -> (arguments of the reference CLI, the same as (epsilon, expected accuracy,
# number of edges, explored edges, batch size) of ngt_refine_anng)
REFINE_A = (["-b", "256"], (0.1, 0.0, 0, INT_MIN, 256))
REFINE_B = (["-e", "0.0", "-k", "15", "-b", "600"], (0.0, 0.0, 15, INT_MIN, 600))
REFINE_B_CASES = ("l1_u8_ties", "ham_u8", "cos_f100")
REFINE_REMOVED_CASE = "l1_f_dups"
ONNG_CASES = ("l1_u8_ties", "ham_u8", "l1_f_dups")
ONNG_ARGS = ["-m", "S", "-s", "n", "-o", "5", "-i", "20"]
ONNG_OUTGOING, ONNG_INCOMING = 5, 20
HUB_NEIGHBOURS = 15
LEAF_AT_LEAST = 5
REFUSED_TAIL = (0, 5000)


def stages_of(name):
    """The stage directories of a case, in the order the recipe makes them."""
    out = ["refine_a"]
    if name in REFINE_B_CASES:
        out.append("refine_b")
    out.append("remove")
    if name == REFINE_REMOVED_CASE:
        out.append("refine_removed")
    if name in ONNG_CASES:
        out.append("onng")
    return out


def sha256(data):
    return hashlib.sha256(data if isinstance(data, bytes) else open(data, "rb").read()).hexdigest()


@functools.lru_cache(maxsize=None)
def expected():
    return json.load(open(os.path.join(GOLD, "stage_matrix.json")))


def fixture_bytes(name, stage, f):
    """The bytes of stage_<name>/<stage>/<f>, unpacked where it is committed gzipped."""
    path = os.path.join(GOLD, "stage_" + name, stage, f)
    if os.path.exists(path + ".gz"):
        with gzip.open(path + ".gz", "rb") as z:
            return z.read()
    return open(path, "rb").read()


def write_fixture(src, dst):
    """Commits one file: as it is, or gzipped with a zero timestamp from GZIP_FROM bytes on."""
    raw = open(src, "rb").read()
    for old in (dst, dst + ".gz"):
        if os.path.exists(old):
            os.remove(old)
    if len(raw) < GZIP_FROM:
        with open(dst, "wb") as f:
            f.write(raw)
        return dst
    with open(dst + ".gz", "wb") as g:
        with gzip.GzipFile(filename="", mode="wb", fileobj=g, mtime=0) as z:
            z.write(raw)
    return dst + ".gz"


@functools.lru_cache(maxsize=None)
def graph(name, stage):
    """(offsets, ids, dists) of a fixture graph, "build" the input's; shared, do not modify."""
    g = F.read_grp(os.path.join(GOLD, "build_" + name, "grp") if stage == "build" else fixture_bytes(name, stage, "grp"))
    for a in g:
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def removed_tree(name):
    c = S.load(name)
    return F.read_tre(fixture_bytes(name, "remove", "tre"), c.dim, c.dtype)


def leaf_lists(tree):
    lo = tree["leaf_off"]
    return [[int(v) for v in tree["leaf_ids"][int(lo[i]):int(lo[i + 1])]] for i in range(len(lo) - 1)]


def valid_after_removal(name, ids=None, outcomes=None):
    """valid[2001] once the ids whose outcome is 1 have left (the fixture's unless given)."""
    if ids is None:
        e = expected()[name]["remove"]
        ids, outcomes = e["ids"], e["removed"]
    valid = np.ones(D.ROWS + 1, np.uint8)
    valid[0] = 0
    for i, ok in zip(ids, outcomes):
        if ok:
            valid[i] = 0
    return valid


def obj_bytes(name, valid=None):
    """The obj file of a case: its rows as the index stores them."""
    c = S.load(name)
    return F.obj_bytes(c.rows, c.dim, valid)


def make_index_dir(name, dst, stage="build"):
    """The index directory a stage starts from, at `dst`: grp, tre and prf of
    build_<name>/ and the written obj; stage "remove": the index after its
    removal (the fixture's grp and tre, obj without the removed rows)."""
    os.makedirs(dst)
    build = os.path.join(GOLD, "build_" + name)
    shutil.copy(os.path.join(build, "prf"), os.path.join(dst, "prf"))
    if stage == "build":
        for f in ("grp", "tre"):
            shutil.copy(os.path.join(build, f), os.path.join(dst, f))
        valid = None
    else:
        assert stage == "remove"
        for f in ("grp", "tre"):
            with open(os.path.join(dst, f), "wb") as out:
                out.write(fixture_bytes(name, "remove", f))
        valid = valid_after_removal(name)
    with open(os.path.join(dst, "obj"), "wb") as out:
        out.write(obj_bytes(name, valid))
    return dst


def restate_refine(name, args, csr, tree=None, valid=None, stats=None):
    """refine_restate.refine of a case with the arguments of ngt_refine_anng."""
    import refine_restate as R
    c = S.load(name)
    eps, acc, k, explore, batch = args
    assert acc == 0.0
    return R.refine(c.rows, c.tree if tree is None else tree, c.prop, csr[0], csr[1], csr[2], eps, k,
                    None if explore == INT_MIN else explore, batch, metric=c.metric, valid=valid, stats=stats)


# ---- the seeds of a query whose leaf a removal emptied ---------------------------------
def glibc_rand(seed):
    """The oracle's restatement of glibc's rand() after srand(seed), as a callable."""
    import ctypes

    import oracle_py as O
    L = O.lib()
    L.ngto_srand.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    L.ngto_rand.argtypes = [ctypes.c_void_p]
    gen = ctypes.create_string_buffer(256)
    L.ngto_srand(gen, seed)
    return lambda: L.ngto_rand(gen)


def random_seeds(rand, graph_empty, seed_size):
    """GraphIndex::getRandomSeeds (lib/NGT/Index.h:775-801): graph_empty[id] is
    true for an id without a graph node."""
    repo = len(graph_empty) - 1
    seed_size = min(seed_size, repo)
    seeds = []
    empty = 0
    while len(seeds) < seed_size:
        r = (float(rand()) + 1.0) / (2147483647.0 + 2.0)
        idx = int(np.floor(repo * r)) + 1
        if graph_empty[idx]:
            empty += 1
            if empty > repo:
                break
            continue
        if idx not in seeds:
            seeds.append(idx)
    return seeds


# ---- the ids a case removes -----------------------------------------------------------
def duplicate_groups(rows):
    """{row bytes: [ids]} of the rows (slot 0 left out) that occur more than once."""
    groups = {}
    for i in range(1, len(rows)):
        groups.setdefault(rows[i].tobytes(), []).append(i)
    return {k: v for k, v in groups.items() if len(v) > 1}


def removal_ids(name, offs, ids, tree, rows):
    """One rule for every case, in this order: the node of the longest list (the
    lowest id among equals); its first 15 neighbours in list order; every id of
    the lowest leaf slot holding at least five ids, ascending; on the tie and
    duplicate cases the lowest id not listed so far whose row has an exact
    duplicate that is not listed either; the first id again; 0; 5000."""
    deg = np.diff(offs.astype(np.int64))
    hub = int(np.argmax(deg))
    out = [hub] + [int(v) for v in ids[int(offs[hub]):int(offs[hub]) + HUB_NEIGHBOURS]]
    leaves = leaf_lists(tree)
    slot = min(i for i, l in enumerate(leaves) if len(l) >= LEAF_AT_LEAST)
    out += sorted(leaves[slot])
    if name in TIE_CASES:
        listed = set(out)
        groups = duplicate_groups(rows)
        out.append(min(min(i for i in g if i not in listed) for g in groups.values()
                       if sum(i not in listed for i in g) >= 2))
    return out + [hub] + list(REFUSED_TAIL)


# ---- what the fixtures exist to test ---------------------------------------------------
def lengths(csr):
    return np.diff(csr[0].astype(np.int64))


def has_list_with_equal_distances(csr):
    offs, _, ds = csr
    o = offs.astype(np.int64)
    return any(len(np.unique(ds[o[v]:o[v + 1]])) < o[v + 1] - o[v] for v in range(1, len(o) - 1))


def check_refine_b(name, a, b):
    la, lb = lengths(a), lengths(b)
    assert lb.max() == 15, (name, "Refine B: the longest list has %d entries" % lb.max())
    assert la.max() > 15, (name, "Refine A has no list longer than 15")


def check_removal(name, entry, rows):
    ids, out = entry["ids"], entry["removed"]
    assert sum(out) >= 20, (name, "fewer than 20 ids removed")
    refused = [i for i, o in zip(ids, out) if not o]
    assert len(refused) >= 3 and refused[-3:] == [ids[0], 0, 5000], (name, refused)
    assert ids[-3] == ids[0]
    if name in TIE_CASES:
        valid = valid_after_removal(name, ids, out)
        groups = duplicate_groups(rows)
        gone = [i for i, o in zip(ids, out) if o]
        assert any(any(valid[j] for j in groups.get(rows[i].tobytes(), [])) for i in gone), \
            (name, "no removed row has a live exact duplicate")


def check_refine_removed(name, csr, valid):
    offs, ids, _ = csr
    assert valid[ids].all(), (name, "the refined graph names a removed id")
    assert (lengths(csr)[valid == 0] == 0).all(), (name, "a removed node has a list")
