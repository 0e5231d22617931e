"""Reference ONNG fixtures: edge and path adjustment of a 2,000-row ANNG.

The first 2,000 rows of tests/golden/sift5k.npy are built into an ANNG with
``ngt create -i t -g a -S 0 -e 0.1 -E 40 -d 128 -o f -D 2`` and reconstructed
with ``ngt reconstruct-graph -s n`` (GraphOptimizer::execute with the three
tuning steps off: GraphReconstructor::reconstructGraph and
adjustPathsEffectively, GraphReconstructor.h:197-561) by the reference CLI
compiled by oracle/ref.mk (oracle/_ref/ngt):

    onng_s   -m s -o 5 -i 40            edge adjustment only
    onng_S   -m S -o 5 -i 40            edge and path adjustment
    onng_E   -m S -E 12 -o 5 -i 40      with a minimum number of edges
    onng_P   -m P                       path adjustment only
    onng_R   -m s -o 30 -i 40 onng_S    non-ANNG input (convertToANNG), short nodes
    onng_R2  -m S -o 8 -i 20 onng_S

Writes ``onng2k/anng/{grp.gz,obj,prf,tre}`` (grp gzip-compressed with a zero
timestamp so that it stays below the 1 MiB limit of a committed file; the
tests unpack it) and ``onng2k/<name>/{grp,prf}``.  Run from the repo root
after build()."""
import argparse
import gzip
import os
import shutil
import subprocess

import numpy as np

ROWS = 2000
CREATE = ["create", "-i", "t", "-g", "a", "-S", "0", "-e", "0.1", "-E", "40", "-d", "128", "-o", "f", "-D", "2"]
# name -> (arguments of reconstruct-graph, input index)
OUTPUTS = [
    ("onng_s", ["-m", "s", "-s", "n", "-o", "5", "-i", "40"], "anng"),
    ("onng_S", ["-m", "S", "-s", "n", "-o", "5", "-i", "40"], "anng"),
    ("onng_E", ["-m", "S", "-s", "n", "-E", "12", "-o", "5", "-i", "40"], "anng"),
    ("onng_P", ["-m", "P", "-s", "n"], "anng"),
    ("onng_R", ["-m", "s", "-s", "n", "-o", "30", "-i", "40"], "onng_S"),
    ("onng_R2", ["-m", "S", "-s", "n", "-o", "8", "-i", "20"], "onng_S"),
]


def run_recipe(ngt, sift_path, work):
    """Runs the recipe in the empty directory `work`; returns it."""
    sift = np.load(sift_path)[:ROWS]
    tsv = os.path.join(work, "sub.tsv")
    with open(tsv, "w") as f:
        for r in sift:
            f.write("\t".join("%d" % v for v in r) + "\n")
    cmds = [CREATE + ["anng", "sub.tsv"]] + [["reconstruct-graph"] + a + [src, name] for name, a, src in OUTPUTS]
    for c in cmds:
        r = subprocess.run([ngt] + c, cwd=work, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("ngt %s failed:\n%s" % (" ".join(c), r.stderr[-2000:]))
    return work


def main():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--work", default="/tmp/ngt_onng_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    run_recipe(args.ngt, os.path.join(args.out, "sift5k.npy"), args.work)
    dst = os.path.join(args.out, "onng2k")
    os.makedirs(os.path.join(dst, "anng"), exist_ok=True)
    for f in ("obj", "prf", "tre"):
        shutil.copy(os.path.join(args.work, "anng", f), os.path.join(dst, "anng", f))
    with open(os.path.join(args.work, "anng", "grp"), "rb") as f, open(os.path.join(dst, "anng", "grp.gz"), "wb") as g:
        with gzip.GzipFile(filename="", mode="wb", fileobj=g, mtime=0) as z:
            z.write(f.read())
    for name, _, _ in OUTPUTS:
        os.makedirs(os.path.join(dst, name), exist_ok=True)
        for f in ("grp", "prf"):
            shutil.copy(os.path.join(args.work, name, f), os.path.join(dst, name, f))
        print(name, "written")


if __name__ == "__main__":
    main()
