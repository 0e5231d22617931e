"""Reference object-removal fixtures: GraphAndTreeIndex::remove (Index.h:1386-1455,
Graph.cpp:641-864 with NGT_FORCED_REMOVE, Tree.h:178-202) through ``ngt remove
<index> ids-file`` of the reference CLI compiled by oracle/ref.mk (oracle/_ref/ngt).

Inputs, all built with the refine recipe's
``ngt create -i t -g a -S 0 -e 0.1 -E 20 -d 128 -o f -D 2``:

    anng   sift5k[:1000]; equal to refine1k/anng (checked), which is reused
    dup    sift5k[:900] followed by sift5k[:100]: objects 901..1000 duplicate 1..100
    tiny   sift5k[:30]: the root is a leaf
    onng   reconstruct-graph -m S -s n -o 10 -i 30 anng onng

Cases (ids in this order):

    rm_one      anng  500
    rm_seq      anng  17, the first 20 neighbours of 17 in list order, 17, 0, 5000
    rm_oneleaf  anng  every id of leaf slot 22, ascending
    rm_all      tiny  1..30
    rm_dup      dup   5, 905, 17, 950, 917
    rm_onng     onng  the node of the longest list, its first 15 neighbours, 3, 4, 5

Every case runs twice and must give byte-identical files; each must differ from
its input in grp, tre and obj and leave prf as it was.  Writes
``remove1k/{dup,tiny}/{grp,obj,prf,tre}``, ``remove1k/onng/{grp,prf}``,
``remove1k/<case>/{grp,tre}`` and ``remove1k/expected.json`` (per case: input,
ids, the per-id outcome read from the CLI's warnings, sha256 of obj and prf).

The CLI runs with OMP_NUM_THREADS=1 (see make_refine_goldens.py).
Run from the repo root after build()."""
import argparse
import filecmp
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ngt_files as F  # noqa: E402

CREATE = ["create", "-i", "t", "-g", "a", "-S", "0", "-e", "0.1", "-E", "20", "-d", "128", "-o", "f", "-D", "2"]
ONNG = ["reconstruct-graph", "-m", "S", "-s", "n", "-o", "10", "-i", "30"]
CASES = [("rm_one", "anng"), ("rm_seq", "anng"), ("rm_oneleaf", "anng"), ("rm_all", "tiny"), ("rm_dup", "dup"),
         ("rm_onng", "onng")]
LEAF_SLOT = 22


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def leaf_ids_of(tre_path, slot):
    t = F.read_tre(tre_path, 128, np.float32)
    return [int(v) for v in t["leaf_ids"][int(t["leaf_off"][slot]):int(t["leaf_off"][slot + 1])]]


def case_ids(name, index_dir):
    offs, ids, _ = F.read_grp(os.path.join(index_dir, "grp"))
    nb = lambda v: [int(x) for x in ids[int(offs[v]):int(offs[v + 1])]]  # noqa: E731
    if name == "rm_one":
        return [500]
    if name == "rm_seq":
        return [17] + nb(17)[:20] + [17, 0, 5000]
    if name == "rm_oneleaf":
        return sorted(leaf_ids_of(os.path.join(index_dir, "tre"), LEAF_SLOT))
    if name == "rm_all":
        return list(range(1, 31))
    if name == "rm_dup":
        return [5, 905, 17, 950, 917]
    if name == "rm_onng":
        deg = np.diff(offs.astype(np.int64))
        hub = int(np.argmax(deg))
        return [hub] + nb(hub)[:15] + [3, 4, 5]
    raise KeyError(name)


def run_recipe(ngt, gold, work):
    """Runs the recipe in the empty directory `work`; returns {case: record}."""
    sift = np.load(os.path.join(gold, "sift5k.npy"))

    def tsv(name, rows):
        with open(os.path.join(work, name), "w") as f:
            for r in rows:
                f.write("\t".join("%d" % v for v in r) + "\n")

    tsv("anng.tsv", sift[:1000])
    tsv("dup.tsv", np.concatenate([sift[:900], sift[:100]]))
    tsv("tiny.tsv", sift[:30])

    def ngt_run(c):
        r = subprocess.run([ngt] + c, cwd=work, capture_output=True, text=True,
                           env=dict(os.environ, OMP_NUM_THREADS="1"))
        if r.returncode != 0:
            raise RuntimeError("ngt %s failed:\n%s" % (" ".join(c), r.stderr[-2000:]))
        return r.stderr

    for name in ("anng", "dup", "tiny"):
        ngt_run(CREATE + [name, name + ".tsv"])
    for f in ("grp", "obj", "prf", "tre"):
        assert filecmp.cmp(os.path.join(work, "anng", f), os.path.join(gold, "refine1k", "anng", f), shallow=False), f
    ngt_run(ONNG + ["anng", "onng"])

    records = {}
    for name, src in CASES:
        ids = case_ids(name, os.path.join(work, src))
        with open(os.path.join(work, name + ".ids"), "w") as f:
            f.write("".join("%d\n" % i for i in ids))
        outcomes = None
        for attempt in ("", ".again"):
            dst = os.path.join(work, name + attempt)
            shutil.copytree(os.path.join(work, src), dst)
            err = ngt_run(["remove", name + attempt, name + ".ids"])
            refused = [int(m) for m in re.findall(r"Warning: Cannot remove the node\. ID=(\d+) ", err)]
            # the warnings name ids, not positions: of an id listed twice the
            # later occurrence is the refused one (it was removed by the first)
            left = {i: refused.count(i) for i in set(refused)}
            out = [1] * len(ids)
            for p in range(len(ids) - 1, -1, -1):
                if left.get(ids[p], 0):
                    left[ids[p]] -= 1
                    out[p] = 0
            assert [i for i, o in zip(ids, out) if not o] == refused, (name, refused)
            assert outcomes is None or outcomes == out, name
            outcomes = out
        for f in ("grp", "obj", "prf", "tre"):
            assert filecmp.cmp(os.path.join(work, name, f), os.path.join(work, name + ".again", f), shallow=False), \
                (name, f, "differs between two runs")
        assert filecmp.cmp(os.path.join(work, name, "prf"), os.path.join(work, src, "prf"), shallow=False), name
        for f in ("grp", "obj", "tre"):
            assert not filecmp.cmp(os.path.join(work, name, f), os.path.join(work, src, f), shallow=False), (name, f)
        records[name] = {"input": src, "ids": ids, "removed": outcomes,
                         "obj_sha256": sha256(os.path.join(work, name, "obj")),
                         "prf_sha256": sha256(os.path.join(work, name, "prf"))}
    return records


def main():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--work", default="/tmp/ngt_remove_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    records = run_recipe(args.ngt, args.out, args.work)
    dst = os.path.join(args.out, "remove1k")
    for name, files in (("dup", ("grp", "obj", "prf", "tre")), ("tiny", ("grp", "obj", "prf", "tre")),
                        ("onng", ("grp", "prf"))):
        os.makedirs(os.path.join(dst, name), exist_ok=True)
        for f in files:
            shutil.copy(os.path.join(args.work, name, f), os.path.join(dst, name, f))
    for name, _ in CASES:
        os.makedirs(os.path.join(dst, name), exist_ok=True)
        for f in ("grp", "tre"):
            shutil.copy(os.path.join(args.work, name, f), os.path.join(dst, name, f))
        print(name, "written")
    with open(os.path.join(dst, "expected.json"), "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
