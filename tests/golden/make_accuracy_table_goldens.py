#!/usr/bin/env python3
"""Reference accuracy tables: Optimizer::generateAccuracyTable
(lib/NGT/Optimizer.h:1495-1573) as `ngt optimize-search-parameters -m a` and
`ngt reconstruct-graph -s a` run it, from the reference CLI compiled by
oracle/ref.mk (oracle/_ref/ngt).

    c1_onng        tests/golden/c1_onng with its table blanked     -m a
    refine1k       tests/golden/refine1k/anng                      -m a
    refine1k_q40   the same                                        -m a -q 40 -n 30
    refine1k_n10   the same                                        -m a -q 50 -n 10   (an error)
    refine1k_onng  reconstruct-graph -m S -s a -o 10 -i 120 of the same
    c1_anng        tests/golden/c1_anng (EdgeSizeForSearch 40)     -m a               (an error)
    acctab_f16     1000 x 16 float32, RandomState(7).rand          -m a
    acctab_u24     1000 x 24 uint8, the same generator's randint   -m a

The two small indexes are created with `ngt create -d <dim> [-o c] -D 2 -E 20
-S 0 -p 1` and committed as acctab_f16/ and acctab_u24/ (grp obj prf tre).
Every case runs three times on fresh copies; the recipe stops when the three
prf files differ (the procedure has one wall-clock clause, Optimizer.h:1461),
and checks that grp, obj and tre stay as they were.  Writes
accuracy_tables.json: per case the AccuracyTable string and the whole prf the
reference wrote, or the error text after the reference's `file:line:` prefixes.

accuracy_trace_c1_onng.bin does not come from the reference: it holds the
search results the restatement (tests/accuracy_restate.py) took from the CPU
oracle, epsilon by epsilon, while it reproduced the c1_onng table, for
tests/cxx/accuracy_table_host.cpp (which documents the layout).  The recipe
refuses to write it unless that table equals the reference's.

Run from the repo root after build()."""
import argparse
import filecmp
import json
import os
import re
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RUNS = 3
CREATE = {
    "acctab_f16": ["create", "-d", "16", "-D", "2", "-E", "20", "-S", "0", "-p", "1"],
    "acctab_u24": ["create", "-d", "24", "-o", "c", "-D", "2", "-E", "20", "-S", "0", "-p", "1"],
}
# name -> (source index, command, arguments before the index path(s))
CASES = [
    ("c1_onng", "c1_onng", "optimize-search-parameters", ["-m", "a"]),
    ("refine1k", "refine1k/anng", "optimize-search-parameters", ["-m", "a"]),
    ("refine1k_q40", "refine1k/anng", "optimize-search-parameters", ["-m", "a", "-q", "40", "-n", "30"]),
    ("refine1k_n10", "refine1k/anng", "optimize-search-parameters", ["-m", "a", "-q", "50", "-n", "10"]),
    ("refine1k_onng", "refine1k/anng", "reconstruct-graph", ["-m", "S", "-s", "a", "-o", "10", "-i", "120"]),
    ("c1_anng", "c1_anng", "optimize-search-parameters", ["-m", "a"]),
    ("acctab_f16", "acctab_f16", "optimize-search-parameters", ["-m", "a"]),
    ("acctab_u24", "acctab_u24", "optimize-search-parameters", ["-m", "a"]),
]


def small_data():
    rs = np.random.RandomState(7)
    return {"acctab_f16": rs.rand(1000, 16).astype(np.float32), "acctab_u24": rs.randint(0, 256, (1000, 24))}


def blank_table(prf):
    lines = [("AccuracyTable\t\n" if l.split("\t")[0] == "AccuracyTable" else l) for l in open(prf)]
    with open(prf, "w") as f:
        f.writelines(lines)


def table_of(prf_text):
    return [l for l in prf_text.split("\n") if l.split("\t")[0] == "AccuracyTable"][0].split("\t")[1]


def error_text(stderr):
    """The message of `ngt: Error <what()>` without the `file:line: ` prefixes."""
    lines = [l for l in stderr.splitlines() if l.startswith("ngt: Error ")]
    assert len(lines) == 1, stderr
    return re.sub(r"\S+\.(?:h|cpp):\d+: ", "", lines[0][len("ngt: Error "):])


def ngt_run(ngt, args, cwd):
    return subprocess.run([ngt] + args, cwd=cwd, capture_output=True, text=True,
                          env=dict(os.environ, OMP_NUM_THREADS="1"))


def run_case(ngt, src, command, args, work):
    """One run on a fresh copy of `src`; returns ('prf', text) or ('error', text)."""
    shutil.rmtree(os.path.join(work, "in"), ignore_errors=True)
    shutil.rmtree(os.path.join(work, "out"), ignore_errors=True)
    shutil.copytree(src, os.path.join(work, "in"))
    blank_table(os.path.join(work, "in", "prf"))
    if command == "reconstruct-graph":
        r = ngt_run(ngt, [command] + args + ["in", "out"], work)
        res = "out"
    else:
        r = ngt_run(ngt, [command] + args + ["in"], work)
        res = "in"
        for f in ("grp", "obj", "tre"):
            assert filecmp.cmp(os.path.join(work, "in", f), os.path.join(src, f), shallow=False), (src, f)
    if "ngt: Error " in r.stderr:
        return "error", error_text(r.stderr)
    if r.returncode != 0:
        raise RuntimeError("ngt %s failed:\n%s" % (command, r.stderr[-2000:]))
    return "prf", open(os.path.join(work, res, "prf")).read()


def create_small_indexes(ngt, work):
    """`ngt create` of acctab_f16 and acctab_u24 under `work` (one thread: no clock, no table)."""
    for name, rows in small_data().items():
        with open(os.path.join(work, name + ".tsv"), "w") as f:
            for r in rows:
                f.write("\t".join(("%d" % v) if name == "acctab_u24" else repr(float(v)) for v in r) + "\n")
        r = ngt_run(ngt, CREATE[name] + [name, name + ".tsv"], work)
        if r.returncode != 0 or not os.path.exists(os.path.join(work, name, "grp")):
            raise RuntimeError("ngt create %s failed:\n%s" % (name, r.stderr[-2000:]))


def run_recipe(ngt, gold, work, cases=CASES):
    """Creates the two small indexes under `work` and runs `cases`; returns {name: {...}}."""
    create_small_indexes(ngt, work)
    out = {}
    for name, src, command, args in cases:
        src_dir = os.path.join(work, src) if src in CREATE else os.path.join(gold, src)
        runs = [run_case(ngt, src_dir, command, args, work) for _ in range(RUNS)]
        if any(r != runs[0] for r in runs):
            raise RuntimeError("%s: the reference's runs differ: %r" % (name, [r[1][:300] for r in runs]))
        kind, text = runs[0]
        entry = {"source": src, "command": "ngt %s %s" % (command, " ".join(args))}
        if kind == "error":
            entry["error"] = text
        else:
            entry["table"] = table_of(text)
            entry["prf"] = text
        out[name] = entry
    return out


def write_trace(gold, table, path):
    """The restatement's per-epsilon search results on c1_onng (100 queries, 20 results)."""
    import struct
    import sys
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    import accuracy_restate as A
    import ngt_files as F
    d = os.path.join(gold, "c1_onng")
    prop = F.read_prf(os.path.join(d, "prf"))
    dim = int(prop["Dimension"])
    rows, valid = F.read_obj(os.path.join(d, "obj"), dim, np.float32)
    offs, ids, _ = F.read_grp(os.path.join(d, "grp"))
    tree = F.read_tre(os.path.join(d, "tre"), dim, np.float32)
    assert rows.shape[0] < 65536
    queries = A.extract_queries(rows, valid, dim, 100)
    trace = []
    pairs, text, maxeps = A.generate(A.oracle_search(rows, tree, prop, offs, ids), rows, valid, prop, 20, 100,
                                     trace=trace)
    if text != table:
        raise RuntimeError("the restatement does not reproduce the reference's c1_onng table")
    out = [b"NGTACCT1", struct.pack("<6I", dim, 2, 20, len(queries), len(trace), len(pairs)),
           queries.astype("<f4").tobytes()]
    for q, size, eps, es, (rid, rd, rn, rc) in trace:
        out.append(struct.pack("<IfiI", size, eps, es, 1 if np.array_equal(q, queries) else 0))
        out += [rn.astype("<u4").tobytes(), rc.astype("<u8").tobytes(), rid.astype("<u2").tobytes(),
                rd.astype("<f4").tobytes()]
    out.append(struct.pack("<f", maxeps))
    out += [struct.pack("<fd", e, a) for e, a in pairs]
    out.append(struct.pack("<I", len(text)) + text.encode())
    with open(path, "wb") as f:
        f.write(b"".join(out))


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--work", default="/tmp/ngt_accuracy_table_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    out = run_recipe(args.ngt, HERE, args.work)
    for name in CREATE:
        os.makedirs(os.path.join(args.out, name), exist_ok=True)
        for f in ("grp", "obj", "prf", "tre"):
            shutil.copy(os.path.join(args.work, name, f), os.path.join(args.out, name, f))
    with open(os.path.join(args.out, "accuracy_tables.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    write_trace(HERE, out["c1_onng"]["table"], os.path.join(args.out, "accuracy_trace_c1_onng.bin"))
    for name, e in sorted(out.items()):
        print(name, e.get("table", e.get("error"))[:100])


if __name__ == "__main__":
    main()
