#!/usr/bin/env python3
"""Reference refine-anng, removal and ONNG fixtures on the construction cases
of tests/build_data.py (GraphReconstructor::refineANNG, GraphAndTreeIndex::remove,
GraphOptimizer::execute), through the reference CLI compiled by oracle/ref.mk
(oracle/_ref/ngt) with OMP_NUM_THREADS=1 (see make_refine_goldens.py).

For each of the nine 2,000-row cases the index is rebuilt from the seeded
generator with the case's own `ngt create` arguments, as make_build_goldens.py
does; grp, tre and prf must equal the committed build_<case>/ files and the
SHA-256 of the reference's obj is recorded.  ncos_f100 starts from the committed
directory as it is: its obj holds the rows the reference normalised, which only
the CPU model that made them reproduces.

    refine_a        every case   refine-anng -b 256: epsilon 0.1, eight batches,
                                 incoming edges
    refine_b        l1_u8_ties, ham_u8, cos_f100
                                 refine-anng -e 0.0 -k 15 -b 600: a size above
                                 EdgeSizeForCreation, no incoming edges, pruned
    remove          every case   remove <index> <ids-file>, the ids of
                                 stage_matrix.removal_ids: the node of the longest
                                 list, its first 15 neighbours in list order, every
                                 id of the lowest leaf slot holding at least five,
                                 on the tie and duplicate cases a row with an exact
                                 duplicate elsewhere, the first id again, 0, 5000
    refine_removed  l1_f_dups    refine_a on the output of its removal
    onng            l1_u8_ties, ham_u8, l1_f_dups
                                 reconstruct-graph -m S -s n -o 5 -i 20

Every command runs twice and must give identical files; every output grp must
differ from its input; a removal must change tre and obj as well and leave prf
alone.  No case had to be left out of a stage: every command was reproducible
on every case.  The conditions the fixtures exist for (stage_matrix.check_*,
and the ties tests/test_stage_matrix_host.py names) are asserted here too, so
that a regenerated fixture cannot quietly stop testing them.

Writes ``stage_<case>/<stage>/grp`` (grp.gz, gzipped with a zero timestamp,
from 900,000 bytes on), ``stage_<case>/remove/tre`` and ``stage_matrix.json``:
per case the SHA-256 of the input obj and per stage the CLI's arguments, the
SHA-256 of the output grp, and for a removal the ids, the per-id outcome read
from the CLI's warnings and the SHA-256 of tre and obj; for onng the GraphType
of the output prf.

Run from the repo root after build()."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import build_data as D  # noqa: E402
import make_build_goldens as B  # noqa: E402
import ngt_files as F  # noqa: E402
import search_matrix as S  # noqa: E402
import stage_matrix as M  # noqa: E402

FILES = ("grp", "obj", "prf", "tre")


def read(path):
    return open(path, "rb").read()


def ngt_run(ngt, work, args):
    r = subprocess.run([ngt] + args, cwd=work, capture_output=True, text=True,
                       env=dict(os.environ, OMP_NUM_THREADS="1"))
    if r.returncode != 0:
        raise RuntimeError("ngt %s failed:\n%s" % (" ".join(args), r.stderr[-2000:]))
    return r.stderr


def outcomes_of(ids, err):
    """Per position 1 (removed) or 0 (refused) from the CLI's warnings.  The
    warnings name ids, not positions: of an id listed twice the later occurrence
    is the refused one (the first removed it)."""
    refused = [int(m) for m in re.findall(r"Warning: Cannot remove the node\. ID=(\d+) ", err)]
    left = {i: refused.count(i) for i in set(refused)}
    out = [1] * len(ids)
    for p in range(len(ids) - 1, -1, -1):
        if left.get(ids[p], 0):
            left[ids[p]] -= 1
            out[p] = 0
    assert [i for i, o in zip(ids, out) if not o] == refused, (ids, refused)
    return out


def same_dirs(work, a, b, what):
    for f in FILES:
        assert read(os.path.join(work, a, f)) == read(os.path.join(work, b, f)), (what, f, "differs between two runs")


def transformed(ngt, work, command, src, dst, what):
    """`ngt <command> src dst`, twice -> dst; prf (unless `command` rewrites it),
    obj and tre stay, grp changes."""
    for out in (dst, dst + ".again"):
        ngt_run(ngt, work, command + [src, out])
    same_dirs(work, dst, dst + ".again", what)
    for f in ("obj", "tre") + (() if command[0] == "reconstruct-graph" else ("prf",)):
        assert read(os.path.join(work, dst, f)) == read(os.path.join(work, src, f)), (what, f)
    assert read(os.path.join(work, dst, "grp")) != read(os.path.join(work, src, "grp")), (what, "grp did not change")
    return {"args": command[1:], "grp_sha256": M.sha256(os.path.join(work, dst, "grp"))}


def run_case(ngt, name, work, log=None):
    """-> (entry of stage_matrix.json, {stage: directory under `work`})."""
    c = S.load(name)
    gold = os.path.join(HERE, "build_" + name)
    if name == "ncos_f100":
        os.makedirs(os.path.join(work, name))
        for f in FILES:
            shutil.copy(os.path.join(gold, f), os.path.join(work, name, f))
    else:
        rows, otype = D.dataset(name)
        B.create(ngt, name, rows, otype, D.CASES[name][3], work)
        for f in ("grp", "tre", "prf"):
            assert read(os.path.join(work, name, f)) == read(os.path.join(gold, f)), \
                "%s: the rebuilt %s differs from the committed one" % (name, f)
    entry = {"obj_sha256": M.sha256(os.path.join(work, name, "obj"))}
    dirs = {}

    def grp(stage):
        return F.read_grp(os.path.join(work, dirs[stage], "grp"))

    dirs["refine_a"] = name + ".refine_a"
    entry["refine_a"] = transformed(ngt, work, ["refine-anng"] + M.REFINE_A[0], name, dirs["refine_a"], (name, "refine_a"))
    if name in M.TIE_CASES:
        assert M.has_list_with_equal_distances(grp("refine_a")), (name, "no refined list holds two equal distances")
        stats = {}
        M.restate_refine(name, M.REFINE_A[1], M.graph(name, "build"), stats=stats)
        assert stats.get("incoming_at_a_present_distance", 0) > 0, \
            (name, "no incoming edge met its distance in the list it went into")
    if name in M.REFINE_B_CASES:
        dirs["refine_b"] = name + ".refine_b"
        entry["refine_b"] = transformed(ngt, work, ["refine-anng"] + M.REFINE_B[0], name, dirs["refine_b"],
                                        (name, "refine_b"))
        M.check_refine_b(name, grp("refine_a"), grp("refine_b"))

    ids = M.removal_ids(name, c.offs, c.ids, c.tree, c.rows)
    with open(os.path.join(work, name + ".ids"), "w") as f:
        f.write("".join("%d\n" % i for i in ids))
    dirs["remove"] = name + ".remove"
    outcomes = None
    for out in (dirs["remove"], dirs["remove"] + ".again"):
        shutil.copytree(os.path.join(work, name), os.path.join(work, out))
        got = outcomes_of(ids, ngt_run(ngt, work, ["remove", out, name + ".ids"]))
        assert outcomes is None or outcomes == got, (name, "outcomes differ between two runs")
        outcomes = got
    same_dirs(work, dirs["remove"], dirs["remove"] + ".again", (name, "remove"))
    assert read(os.path.join(work, dirs["remove"], "prf")) == read(os.path.join(work, name, "prf")), (name, "remove")
    for f in ("grp", "obj", "tre"):
        assert read(os.path.join(work, dirs["remove"], f)) != read(os.path.join(work, name, f)), (name, "remove", f)
    entry["remove"] = {"ids": ids, "removed": outcomes}
    for f in ("grp", "tre", "obj"):
        entry["remove"][f + "_sha256"] = M.sha256(os.path.join(work, dirs["remove"], f))
    M.check_removal(name, entry["remove"], c.rows)

    if name == M.REFINE_REMOVED_CASE:
        dirs["refine_removed"] = name + ".refine_removed"
        entry["refine_removed"] = transformed(ngt, work, ["refine-anng"] + M.REFINE_A[0], dirs["remove"],
                                              dirs["refine_removed"], (name, "refine_removed"))
        M.check_refine_removed(name, grp("refine_removed"), M.valid_after_removal(name, ids, outcomes))
    if name in M.ONNG_CASES:
        dirs["onng"] = name + ".onng"
        entry["onng"] = transformed(ngt, work, ["reconstruct-graph"] + M.ONNG_ARGS, name, dirs["onng"], (name, "onng"))
        entry["onng"]["graph_type"] = F.read_prf(os.path.join(work, dirs["onng"], "prf"))["GraphType"]
    assert list(dirs) == M.stages_of(name)
    if log:
        log("%s: %s" % (name, ", ".join(dirs)))
    return entry, dirs


def committed_files(name):
    """[(stage, file)] of what a case commits."""
    return [(s, f) for s in M.stages_of(name) for f in (("grp", "tre") if s == "remove" else ("grp",))]


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--work", default="/tmp/ngt_stage_matrix_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    records = {}
    total = 0
    for name in M.CASES:
        records[name], dirs = run_case(args.ngt, name, args.work, log=print)
        for stage, f in committed_files(name):
            dst = os.path.join(args.out, "stage_" + name, stage)
            os.makedirs(dst, exist_ok=True)
            path = M.write_fixture(os.path.join(args.work, dirs[stage], f), os.path.join(dst, f))
            size = os.path.getsize(path)
            assert size < M.MAX_FILE, (path, size)
            total += size
            print("  %-44s %8d bytes" % (os.path.relpath(path, args.out), size))
    path = os.path.join(args.out, "stage_matrix.json")
    with open(path, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d bytes of fixtures and %d of json" % (total, os.path.getsize(path)))


if __name__ == "__main__":
    main()
