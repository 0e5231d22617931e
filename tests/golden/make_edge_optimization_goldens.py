#!/usr/bin/env python3
"""Reference results of `ngt optimize-#-of-edges`
(GraphOptimizer::optimizeNumberOfEdgesForANNG, lib/NGT/GraphOptimizer.h:386-543)
from the reference CLI compiled by oracle/ref.mk (oracle/_ref/ngt).

The data is not committed: tests/edges_data.py generates it (f16: 25,400 x 16
float32, u8: 25,400 x 16 uint8, u8_3000: the first 3,000 rows of u8).  Each data
set is written as text and indexed with `ngt create -d 16 -D 2 [-o c]`; the
procedure discards graph and tree, so only obj and prf matter to it.

Every case runs three times on fresh copies of its index; the recipe stops when
the three runs differ (printed line, prf or error text) or when grp, obj or tre
change.  Writes edge_optimization.json: per case the data set, the arguments,
the printed `The optimized # of edges=N(acc)` line and the whole prf the
reference wrote, or the error text after the reference's `file:line:`
prefixes together with the (unchanged) prf.  The CPU seconds of each run go to
the log only.

Run from the repo root after build()."""
import argparse
import filecmp
import json
import os
import re
import resource
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edges_data as D  # noqa: E402

RUNS = 3
# name -> (data set, arguments)
CASES = [
    ("A", "f16", ["-a", "0.99", "-e", "30", "-q", "50", "-k", "20"]),
    ("B", "f16", ["-a", "0.95", "-o", "1000000", "-q", "100", "-k", "10"]),
    ("C", "f16", []),
    ("D", "f16", ["-o", "12500"]),
    ("E", "f16", ["-o", "25000"]),
    ("F", "f16", ["-a", "0.99", "-o", "1000000"]),
    ("G", "f16", ["-a", "0.97", "-o", "25000"]),
    ("H", "u8", ["-a", "0.95", "-e", "40", "-q", "50", "-k", "20"]),
    ("X1", "u8_3000", []),
    ("X2", "u8_3000", ["-q", "4000"]),
]


def error_text(stderr):
    """The message of `ngt: Error: <what()>` without the `file:line: ` prefixes."""
    lines = [l for l in stderr.splitlines() if l.startswith("ngt: Error: ")]
    assert len(lines) == 1, stderr
    return re.sub(r"\S+\.(?:h|cpp):\d+: ", "", lines[0][len("ngt: Error: "):])


def ngt_run(ngt, args, cwd):
    before = resource.getrusage(resource.RUSAGE_CHILDREN)
    r = subprocess.run([ngt] + args, cwd=cwd, capture_output=True, text=True)
    after = resource.getrusage(resource.RUSAGE_CHILDREN)
    cpu = (after.ru_utime + after.ru_stime) - (before.ru_utime + before.ru_stime)
    return r, cpu


def create_index(ngt, name, work):
    rows, otype = D.dataset(name)
    D.write_text(rows, otype, os.path.join(work, name + ".tsv"))
    args = ["create", "-d", str(D.DIM), "-D", "2"] + (["-o", "c"] if otype == "c" else [])
    r, _ = ngt_run(ngt, args + [name, name + ".tsv"], work)
    if r.returncode != 0 or not os.path.exists(os.path.join(work, name, "grp")):
        raise RuntimeError("ngt create %s failed:\n%s" % (name, r.stderr[-2000:]))


def run_case(ngt, src, args, work):
    """One run on a fresh copy of `src`: (printed line or None, error or None, prf text), CPU seconds."""
    dst = os.path.join(work, "in")
    shutil.rmtree(dst, ignore_errors=True)
    shutil.copytree(src, dst)
    r, cpu = ngt_run(ngt, ["optimize-#-of-edges"] + args + ["in"], work)
    for f in ("grp", "obj", "tre"):
        assert filecmp.cmp(os.path.join(dst, f), os.path.join(src, f), shallow=False), (src, f)
    prf = open(os.path.join(dst, "prf")).read()
    if "ngt: Error: " in r.stderr:
        return (None, error_text(r.stderr), prf), cpu
    lines = [l for l in r.stdout.splitlines() if l.startswith("The optimized # of edges=")]
    if r.returncode != 0 or len(lines) != 1:
        raise RuntimeError("ngt optimize-#-of-edges failed:\n%s\n%s" % (r.stdout[-2000:], r.stderr[-2000:]))
    return (lines[0], None, prf), cpu


def run_recipe(ngt, work, cases=CASES, log=None):
    out = {}
    made = set()
    for name, data, args in cases:
        if data not in made:
            create_index(ngt, data, work)
            made.add(data)
        src = os.path.join(work, data)
        runs, cpus = [], []
        for _ in range(RUNS):
            res, cpu = run_case(ngt, src, args, work)
            runs.append(res)
            cpus.append(round(cpu, 2))
        if any(r != runs[0] for r in runs):
            raise RuntimeError("%s: the reference's runs differ: %r" % (name, [(r[0], r[1]) for r in runs]))
        line, error, prf = runs[0]
        entry = {"data": data, "args": args, "prf": prf}
        if error is not None:
            entry["error"] = error
            assert prf == open(os.path.join(src, "prf")).read(), name
        else:
            entry["line"] = line
        out[name] = entry
        if log:
            log("%s %s -> %s (CPU s %s)" % (name, " ".join(args), line or error, cpus))
    return out


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--work", default="/tmp/ngt_edge_optimization_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    out = run_recipe(args.ngt, args.work, log=print)
    with open(os.path.join(args.out, "edge_optimization.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
