#!/usr/bin/env python3
"""Reference searches of the construction cases of tests/build_data.py.

For each of the nine 2,000-row cases the reference CLI (oracle/_ref/ngt,
compiled by oracle/ref.mk) rebuilds the index as make_build_goldens.py does,
the rebuilt grp and tre are compared byte for byte with the committed
build_<case>/{grp,tre}, and `ngt search -o e` runs on the 32 queries of
build_data.queries() in these modes:

  t10r, t10w  -i t -n 10 -e 0.1, index opened read-only and read-write
  t50, t50w   -i t -n 50 -e 0.02, read-only (the CLI's default) and read-write
  s10         -i s -n 10
  s40r        -i s -n 40 -r <radius>

<radius> is the median over the queries of the 10th-nearest distance of the
CPU restatement's linear search (tests/search_matrix.py), a float32.  Writes
build_<case>/search.npz: per mode <mode>_ids [32, k] (-1 behind the last
result), <mode>_dists [32, k] (the printed distances, NaN behind the last) and
<mode>_ndist [32], and the radius.

ncos_f100's objects are normalised by the reference with the CPU's
reciprocal-square-root approximation: on another CPU
model than the one that made the committed files the rebuilt index differs,
and the searches run on the committed obj, grp and tre instead.

An index opened read-only walks its graph by a table of distances that has no
entry for Angle on uint8 rows and uses L2 there (tests/search_matrix.py,
read_only_metric): ang_u8's t10r and t50 are L2 results, t10w and t50w Angle.

Run from the repo root after build()."""
import argparse
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import build_data as D  # noqa: E402
import make_build_goldens as B  # noqa: E402
import ngt_files as F  # noqa: E402
import search_matrix as S  # noqa: E402

MAX_FILE = 1000000


def modes(radius):
    """key -> (k, arguments of `ngt search`)."""
    return {
        "t10r": (10, ["-i", "t", "-n", "10", "-e", "0.1", "-m", "r"]),
        "t10w": (10, ["-i", "t", "-n", "10", "-e", "0.1", "-m", "w"]),
        "t50": (50, ["-i", "t", "-n", "50", "-e", "0.02"]),
        "t50w": (50, ["-i", "t", "-n", "50", "-e", "0.02", "-m", "w"]),
        "s10": (10, ["-i", "s", "-n", "10"]),
        "s40r": (40, ["-i", "s", "-n", "40", "-r", "%.9g" % radius]),
    }


def read(path):
    return open(path, "rb").read()


def run_case(ngt, name, work, log=None):
    """-> the arrays of build_<name>/search.npz."""
    _, o, _, batch = D.CASES[name]
    rows, otype = D.dataset(name)
    index = B.create(ngt, name, rows, otype, batch, work)
    gold = os.path.join(HERE, "build_" + name)
    same = all(read(os.path.join(index, f)) == read(os.path.join(gold, f)) for f in ("grp", "tre"))
    if not same:
        if name != "ncos_f100":
            raise RuntimeError("%s: the rebuilt grp / tre differ from the committed ones" % name)
        if log:
            log("%s: rebuilt on another CPU model; searching the committed files" % name)
        for f in ("obj", "grp", "tre"):
            shutil.copy(os.path.join(gold, f), os.path.join(index, f))
    qs = D.queries(name)
    tsv = os.path.join(work, name + "_queries.tsv")
    D.write_text(qs, otype, tsv)
    radius = np.float32(S.fixture_radius(name))
    out = {"radius": radius}
    for key, (k, args) in modes(radius).items():
        r = subprocess.run([ngt, "search"] + args + ["-o", "e", name, tsv], cwd=work, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("ngt search %s %s failed:\n%s\n%s" % (name, key, r.stdout[-2000:], r.stderr[-2000:]))
        res = F.parse_search_output(r.stdout)
        assert len(res) == len(qs), (name, key, len(res))
        ids = np.full((len(res), k), -1, np.int32)
        dists = np.full((len(res), k), np.nan, np.float64)
        for i, q in enumerate(res):
            ids[i, :len(q["ids"])] = q["ids"]
            dists[i, :len(q["dists"])] = q["dists"]
        out[key + "_ids"], out[key + "_dists"] = ids, dists
        out[key + "_ndist"] = np.array([q["ndist"] for q in res], np.int64)
    return out


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngt", default=os.path.join(root, "oracle", "_ref", "ngt"))
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--work", default="/tmp/ngt_search_matrix_goldens")
    args = ap.parse_args()
    shutil.rmtree(args.work, ignore_errors=True)
    os.makedirs(args.work)
    for name in S.CASES:
        arrays = run_case(args.ngt, name, args.work, log=print)
        path = os.path.join(args.out, "build_" + name, "search.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < MAX_FILE, (name, os.path.getsize(path))
        print("%s written: radius %.9g, %d bytes" % (name, arrays["radius"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
