#!/usr/bin/env python3
"""Reference builds of the graph-type cases of tests/graph_type_data.py.

Each case is `ngt create -g k|i|o` of its generated rows with the reference CLI
compiled by oracle/ref.mk (oracle/_ref/ngt); the incremental case is `ngt
create` of its first rows and `ngt append` of the rest.  KNNG runs with one
creation thread (-p 1): with more the reference inserts a batch into the DVP
tree in thread completion order and its tre does not repeat.  Writes
gtype_<type>_<case>/{grp,tre,prf}.

Every command runs twice in fresh directories; a case whose grp or tre differs
between the two runs is not written, and the recipe fails naming it.

Run from the repo root after build()."""
import argparse
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import build_data as D  # noqa: E402
import graph_type_data as G  # noqa: E402

MAX_FILE = 1000000


def run(ngt, args, work):
    r = subprocess.run([ngt] + args, cwd=work, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("ngt %s failed (%d):\n%s\n%s" % (" ".join(args), r.returncode, r.stdout[-2000:],
                                                           r.stderr[-2000:]))


def create(ngt, case, name, work):
    """The case's reference commands in a fresh directory -> the index directory."""
    shutil.rmtree(os.path.join(work, name), ignore_errors=True)
    rows, otype = D.dataset(case["data"])
    cut = case["cut"] or len(rows)
    tsv = os.path.join(work, name + ".tsv")
    D.write_text(rows[:cut], otype, tsv)
    run(ngt, G.create_args(case) + [name, tsv], work)
    if cut < len(rows):
        more = os.path.join(work, name + ".more.tsv")
        D.write_text(rows[cut:], otype, more)
        run(ngt, ["append", "-p", str(case["threads"]), name, more], work)
    if not os.path.exists(os.path.join(work, name, "grp")):
        raise RuntimeError("%s: no grp written" % name)
    return os.path.join(work, name)


def run_recipe(ngt, work, out, log=None):
    unstable = []
    for case in G.CASES:
        a = create(ngt, case, case["dir"] + "_a", work)
        b = create(ngt, case, case["dir"] + "_b", work)
        differ = [f for f in ("grp", "tre")
                  if open(os.path.join(a, f), "rb").read() != open(os.path.join(b, f), "rb").read()]
        if differ:
            unstable.append((case["dir"], differ))
            if log:
                log("%s NOT written: %s differ between two runs" % (case["dir"], differ))
            continue
        dst = os.path.join(out, case["dir"])
        os.makedirs(dst, exist_ok=True)
        for f in ("grp", "tre", "prf"):
            size = os.path.getsize(os.path.join(a, f))
            assert size < MAX_FILE, (case["dir"], f, size)
            shutil.copy(os.path.join(a, f), os.path.join(dst, f))
        if log:
            log("%s written: grp %d bytes" % (case["dir"], os.path.getsize(os.path.join(a, "grp"))))
    return unstable


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--work", default="/tmp/ngt_graph_type_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    unstable = run_recipe(args.ngt, args.work, args.out, log=print)
    if unstable:
        raise SystemExit("not repeatable, left out: %s" % unstable)


if __name__ == "__main__":
    main()
