"""Reference refine-anng fixtures: GraphReconstructor::refineANNG
(GraphReconstructor.h:803-924) on a 1,000-row ANNG.

The first 1,000 rows of tests/golden/sift5k.npy are built into an ANNG with
``ngt create -i t -g a -S 0 -e 0.1 -E 20 -d 128 -o f -D 2`` and refined with
``ngt refine-anng`` by the reference CLI compiled by oracle/ref.mk
(oracle/_ref/ngt):

    r_b256   -e 0.0 -b 256              four batches, incoming edges
    r_one    -e 0.0                     one batch; differs from r_b256
    r_k10    -e 0.0 -k 10 -b 100        kNN graph: no incoming edges, pruned
    r_k30    -e 0.0 -k 30 -b 256        size above EdgeSizeForCreation
    r_km30   -e 0.0 -k -30 -b 256       negative k: no incoming, no prune
    r_E10    -e -0.1 -E 10 -b 256       explored-edge limit, a hub of 484
    r_a      -a 0.8 -b 256 on anng_t    expected accuracy

anng_t is anng with the AccuracyTable line of tests/golden/c1_onng/prf in its
prf.  Writes ``refine1k/anng/{grp,obj,prf,tre}``, ``refine1k/anng_t/prf`` and
``refine1k/<name>/grp``; refine-anng leaves prf, obj and tre as they were, which
the recipe checks.  It also checks that r_b256 and r_one differ, so that a
regenerated fixture cannot silently stop testing the batch order.

The CLI runs with OMP_NUM_THREADS=1.  refineANNG searches a batch with an
OpenMP loop, and getSeedsFromTree thins a leaf's seeds with srand(leaf id) and
rand(), whose state all threads share: with several threads the seeds of a
search depend on the interleaving.  Well-searched settings hide that (r_b256 is
the same with 1 or 8 threads), the sparse searches of r_E10 do not: its grp
changed from run to run with the default thread count.  One thread is the
sequence the code itself defines, and the only reproducible one.

Run from the repo root after build()."""
import argparse
import filecmp
import os
import shutil
import subprocess

import numpy as np

ROWS = 1000
CREATE = ["create", "-i", "t", "-g", "a", "-S", "0", "-e", "0.1", "-E", "20", "-d", "128", "-o", "f", "-D", "2"]
# name -> (arguments of refine-anng, input index)
OUTPUTS = [
    ("r_b256", ["-e", "0.0", "-b", "256"], "anng"),
    ("r_one", ["-e", "0.0"], "anng"),
    ("r_k10", ["-e", "0.0", "-k", "10", "-b", "100"], "anng"),
    ("r_k30", ["-e", "0.0", "-k", "30", "-b", "256"], "anng"),
    ("r_km30", ["-e", "0.0", "-k", "-30", "-b", "256"], "anng"),
    ("r_E10", ["-e", "-0.1", "-E", "10", "-b", "256"], "anng"),
    ("r_a", ["-a", "0.8", "-b", "256"], "anng_t"),
]


def with_accuracy_table(prf_in, table_prf, prf_out):
    table = [l for l in open(table_prf) if l.split("\t")[0] == "AccuracyTable"]
    assert len(table) == 1 and table[0].split("\t")[1].strip()
    lines = [l for l in open(prf_in) if l.split("\t")[0] != "AccuracyTable"] + table
    with open(prf_out, "w") as f:
        f.writelines(sorted(lines))


def run_recipe(ngt, gold, work):
    """Runs the recipe in the empty directory `work`; returns it."""
    sift = np.load(os.path.join(gold, "sift5k.npy"))[:ROWS]
    with open(os.path.join(work, "sub.tsv"), "w") as f:
        for r in sift:
            f.write("\t".join("%d" % v for v in r) + "\n")

    def ngt_run(c):
        r = subprocess.run([ngt] + c, cwd=work, capture_output=True, text=True,
                           env=dict(os.environ, OMP_NUM_THREADS="1"))
        if r.returncode != 0:
            raise RuntimeError("ngt %s failed:\n%s" % (" ".join(c), r.stderr[-2000:]))

    ngt_run(CREATE + ["anng", "sub.tsv"])
    shutil.copytree(os.path.join(work, "anng"), os.path.join(work, "anng_t"))
    with_accuracy_table(os.path.join(work, "anng", "prf"), os.path.join(gold, "c1_onng", "prf"),
                        os.path.join(work, "anng_t", "prf"))
    for name, a, src in OUTPUTS:
        ngt_run(["refine-anng"] + a + [src, name])
        for f in ("prf", "obj", "tre"):
            assert filecmp.cmp(os.path.join(work, name, f), os.path.join(work, src, f), shallow=False), (name, f)
        assert not filecmp.cmp(os.path.join(work, name, "grp"), os.path.join(work, src, "grp"), shallow=False), name
    assert not filecmp.cmp(os.path.join(work, "r_b256", "grp"), os.path.join(work, "r_one", "grp"), shallow=False), \
        "the batch size no longer changes the result: choose other parameters"
    return work


def main():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--work", default="/tmp/ngt_refine_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    run_recipe(args.ngt, args.out, args.work)
    dst = os.path.join(args.out, "refine1k")
    os.makedirs(os.path.join(dst, "anng"), exist_ok=True)
    os.makedirs(os.path.join(dst, "anng_t"), exist_ok=True)
    for f in ("grp", "obj", "prf", "tre"):
        shutil.copy(os.path.join(args.work, "anng", f), os.path.join(dst, "anng", f))
    shutil.copy(os.path.join(args.work, "anng_t", "prf"), os.path.join(dst, "anng_t", "prf"))
    for name, _, _ in OUTPUTS:
        os.makedirs(os.path.join(dst, name), exist_ok=True)
        shutil.copy(os.path.join(args.work, name, "grp"), os.path.join(dst, name, "grp"))
        print(name, "written")


if __name__ == "__main__":
    main()
