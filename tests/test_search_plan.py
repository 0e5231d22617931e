"""The search launch planning (ngt_amd/csrc/search_plan.cpp) is pure host
arithmetic: which kernel a shape gets, with which LDS capacities.  A
stand-alone program (tests/cxx/search_plan_table.cpp, linking only
search_plan.cpp) prints one line per case, the inputs and every field of the
plan; the output is compared with tests/golden/search_plan_table.txt,
recorded when the planning moved out of run_search unchanged.  The golden
file holds the hand-derived and the per-knob rows as printed, and the cross
product packed: every distinct plan once, then per (metric, dp, nq, k) the
plan numbers of its 96 cases.  No device call is made here."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngt_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "search_plan_table.txt")
CROSS = "# the cross product, no knobs"
PER_LINE = 96  # visited_hash_log2 x distance_filter x (adj_stride, edge_size) x lds_per_block


def cross_inputs():
    """The cross product's cases in the order the program prints them."""
    for m, dp, nq, k, vis, filt, adj, lds in itertools.product(
            ("L2", "cos"), (96, 128, 960), (1, 200, 600, 10000), (10, 100, 500), (0, 12, -1, -2), (-1, 0, 1),
            ("0/40", "40/40", "256/136", "512/300"), (65536, 163840)):
        yield "%s %d %d %d %d %d %s %d 100000 -" % (m, dp, nq, k, vis, filt, adj, lds)


def pack(lines):
    """The program's output in the golden file's form."""
    at = lines.index(CROSS)
    cases = [l.split(" | ") for l in lines[at + 1:]]
    assert [c[0] for c in cases] == list(cross_inputs())
    plans = []
    for _, p in cases:
        if p not in plans:
            plans.append(p)
    out = lines[:at] + ["# the distinct plans of the cross product"]
    out += ["%d | %s" % (i, p) for i, p in enumerate(plans)]
    out.append(CROSS + ": metric dp nq k : the plans of visited_hash_log2 0 12 -1 -2 x distance_filter -1 0 1 x "
               "adj_stride/edge_size 0/40 40/40 256/136 512/300 x lds_per_block 65536 163840 (innermost)")
    for i in range(0, len(cases), PER_LINE):
        out.append(" ".join(cases[i][0].split()[:4]) + " : " +
                   " ".join(str(plans.index(p)) for _, p in cases[i:i + PER_LINE]))
    return out


def plan_of(lines, inputs):
    hits = [l.split(" | ")[1].split() for l in lines if l.startswith(inputs + " - | ")]
    assert hits, inputs
    return hits[0]


def test_plan_table_matches_golden(tmp_path):
    exe = str(tmp_path / "search_plan_table")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "search_plan_table.cpp"),
                           os.path.join(CSRC, "search_plan.cpp")])
    lines = subprocess.check_output([exe]).decode().splitlines()
    got = pack(lines)
    want = open(GOLDEN).read().splitlines()
    diff = [(i + 1, w, g) for i, (w, g) in enumerate(itertools.zip_longest(want, got)) if w != g]
    assert not diff, diff[:5]

    # the rows derived by hand from run_search before the planning moved:
    # kernel, ht / cq / vf, accepted only, filter, LDS bytes, sched shape
    def key(p):
        return (p[0], int(p[1]), int(p[2]), int(p[3]), int(p[4]), int(p[6]), int(p[14]), int(p[15]))
    assert key(plan_of(lines, "cos 128 1000 10 0 0 40/40 65536 100000")) == ("one", 13, 3072, 15, 0, 0, 62944, 0)
    assert key(plan_of(lines, "cos 128 200 10 0 0 40/40 163840 100000")) == ("one", 14, 8192, 15, 0, 0, 137312, 0)
    assert key(plan_of(lines, "cos 128 1000 500 0 0 40/40 65536 100000")) == ("one", 12, 1024, 0, 0, 0, 29744, 0)
    assert key(plan_of(lines, "L2 128 10000 10 -2 0 256/136 65536 100000")) == ("one", 0, 512, 15, 1, 1, 9760, 1)
    p = plan_of(lines, "L2 128 10000 10 -2 0 40/40 65536 100000")
    assert key(p)[:6] == ("law", 0, 256, 14, 1, 1) and p[7:10] == ["80", "8", "0"] and p[15] == "0"
    p = plan_of(lines, "L2 128 1 10 0 0 40/40 163840 100000")          # the visited bitmap fits
    assert (p[0], p[3], p[6], p[15]) == ("spec", "15", "1", "0")
    p = plan_of(lines, "L2 128 1 10 0 0 40/40 163840 10000000")        # ... and does not
    assert (p[0], p[2], p[3], p[6], p[7], p[8], p[15]) == ("la8", "2048", "15", "1", "2048", "12", "0")
