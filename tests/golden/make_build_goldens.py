#!/usr/bin/env python3
"""Reference builds of the construction cases of tests/build_data.py.

Each case is `ngt create -d <dim> -D <distance> -o <type> -b <batch>` of its
generated rows with the reference CLI compiled by oracle/ref.mk
(oracle/_ref/ngt).  Writes build_<case>/{grp,tre,prf} (and obj for ncos_f100,
whose objects the reference normalises), and build_cases.json with each case's
row count and batch size.  The reference's normalisation starts from the CPU's
reciprocal-square-root approximation, so ncos_f100's obj, grp and tre come out the
same only on the CPU model that made them.

l2_f4_onebatch is one creation batch of all its rows: 30,000, or the next
multiple of 5,000 at which the reference tree has at least 300 internal nodes.
Only its tre is written; build_cases.json records the SHA-256 of its grp.

Run from the repo root after build()."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import build_data as D  # noqa: E402
import ngt_files as F  # noqa: E402

MAX_FILE = 1000000


def create(ngt, name, rows, otype, batch, work):
    """`ngt create` of `rows` in a fresh directory -> the index directory."""
    shutil.rmtree(os.path.join(work, name), ignore_errors=True)
    tsv = os.path.join(work, name + ".tsv")
    D.write_text(rows, otype, tsv)
    r = subprocess.run([ngt] + D.create_args(name, batch) + [name, tsv], cwd=work, capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(os.path.join(work, name, "grp")):
        raise RuntimeError("ngt create %s failed:\n%s\n%s" % (name, r.stdout[-2000:], r.stderr[-2000:]))
    return os.path.join(work, name)


def run_case(ngt, name, work, log=None):
    """-> (index directory, entry of build_cases.json, files to commit)."""
    _, o, dim, batch = D.CASES[name]
    if name != "l2_f4_onebatch":
        rows, otype = D.dataset(name)
        src = create(ngt, name, rows, otype, batch, work)
        files = ["grp", "tre", "prf"] + (["obj"] if name == "ncos_f100" else [])
        return src, {"rows": len(rows), "batch": batch}, files
    n = D.ONEBATCH_FIRST_ROWS
    while True:
        rows, otype = D.dataset(name, n)
        src = create(ngt, name, rows, otype, n, work)
        tree = F.read_tre(os.path.join(src, "tre"), dim, np.float32)
        internal = int(tree["in_valid"].sum())
        if log:
            log("%s: %d rows -> %d internal nodes" % (name, n, internal))
        if internal >= D.ONEBATCH_MIN_INTERNAL:
            break
        n += D.ONEBATCH_STEP
    sha = hashlib.sha256(open(os.path.join(src, "grp"), "rb").read()).hexdigest()
    return src, {"rows": n, "batch": n, "grp_sha256": sha}, ["tre"]


def run_recipe(ngt, work, out, names=None, log=None):
    cases = {}
    for name in names or D.CASES:
        src, entry, files = run_case(ngt, name, work, log)
        dst = os.path.join(out, "build_" + name)
        os.makedirs(dst, exist_ok=True)
        for f in files:
            size = os.path.getsize(os.path.join(src, f))
            assert size < MAX_FILE, (name, f, size)
            shutil.copy(os.path.join(src, f), os.path.join(dst, f))
        cases[name] = entry
        if log:
            log("%s written: %s" % (name, entry))
    return cases


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--work", default="/tmp/ngt_build_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    cases = run_recipe(args.ngt, args.work, args.out, log=print)
    with open(os.path.join(args.out, "build_cases.json"), "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
