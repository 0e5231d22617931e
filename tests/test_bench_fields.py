"""bench.py's roofline fields (CPU): SURVEY.md 8(d)'s literal bytes, the
Infinity-Cache-resident share and the counter-based bound label."""
import numpy as np

import bench


def test_literal_bytes_exact_and_qg():
    # counters [q, 8]: c[0] distances, c[4] edges (exact) / code blocks (qg), c[3] exact distances (qg)
    c = np.zeros((3, 8))
    c[:, 0] = [100, 200, 300]
    c[:, 4] = [10, 20, 30]
    c[:, 3] = [5, 5, 5]
    dp, nq, k = 128, 3, 10
    assert bench.literal_bytes(c, dp, nq, k, False, 128) == 600 * dp * 4 + 60 * 4 + nq * (dp * 4 + k * 8)
    # NGTQG: blocks * 8 * Me + ADC distances * 4 + exact rows * Dp * 4 + per query Dp * 4 + k * 8
    assert bench.literal_bytes(c, dp, nq, k, True, 128) == 60 * 8 * 128 + 600 * 4 + 15 * dp * 4 + nq * (dp * 4 + k * 8)


def test_ic_share():
    assert bench.ic_share(None, 100.0) == 0.0
    assert bench.ic_share({"filter_copy_fits_infinity_cache": False, "filter_copy_bytes": 50.0}, 100.0) == 0.0
    assert bench.ic_share({"filter_copy_fits_infinity_cache": True, "filter_copy_bytes": 88.0}, 100.0) == 0.88


def test_bound_from_counters():
    w = 1000.0
    assert bench.bound_from_counters({"SQ_WAVE_CYCLES": w, "SQ_WAIT_ANY": 560, "SQ_ACTIVE_INST_VALU": 100}) == "latency"
    assert bench.bound_from_counters({"SQ_WAVE_CYCLES": w, "SQ_WAIT_ANY": 300, "SQ_ACTIVE_INST_VALU": 600}) == "valu"
    assert bench.bound_from_counters({"SQ_WAVE_CYCLES": w, "SQ_WAIT_ANY": 300, "SQ_ACTIVE_INST_VALU": 100}) == "hbm"
    # most algorithmic bytes from an Infinity-Cache-resident table (the C2 filter copy)
    assert bench.bound_from_counters({"SQ_WAVE_CYCLES": w, "SQ_WAIT_ANY": 495, "SQ_ACTIVE_INST_VALU": 100},
                                     0.90) == "infinity-cache"
    assert bench.bound_from_counters({"SQ_WAVE_CYCLES": w, "SQ_WAIT_ANY": 560, "SQ_ACTIVE_INST_VALU": 100},
                                     0.90) == "latency"


def test_run_reaped_terminates_leftovers(tmp_path):
    """A child's own leftovers (here a background sleep it does not wait for)
    are terminated with its process group once it exits."""
    import time
    pidfile = tmp_path / "pid"
    rc, out, _ = bench.run_reaped(["bash", "-c", "sleep 60 & echo $! > %s; echo done" % pidfile], 30,
                                  capture_stderr=True, what="test child")
    assert rc == 0 and out.strip() == "done"
    pid = int(pidfile.read_text())
    for _ in range(50):
        try:
            with open("/proc/%d/stat" % pid) as f:
                state = f.read().rsplit(")", 1)[1].split()[0]
        except OSError:
            break
        if state == "Z":
            break
        time.sleep(0.1)
    else:
        raise AssertionError("the leftover sleep survived its group")


def test_bound_issue_from_clocked_pass():
    """A SIMD issuing in >= 0.7 of its measured cycles is issue-bound even when
    its waves wait on memory most of the time (the other waves fill in)."""
    w = 1000.0
    cn = {"SQ_WAVE_CYCLES": w, "SQ_WAIT_ANY": 650, "SQ_ACTIVE_INST_VALU": 150}
    assert bench.bound_from_counters(cn, 0.0, {"simd_issue_util": 0.78}) == "issue"
    assert bench.bound_from_counters(cn, 0.0, {"simd_issue_util": 0.58}) == "latency"
    assert bench.bound_from_counters(cn, 0.0, None) == "latency"


def test_pick_expansion():
    sw = [{"result_expansion": 2.0, "epsilon": 0.106, "recall_at_10": 0.955, "kernel_ms": 85.0},
          {"result_expansion": 3.0, "epsilon": 0.098, "recall_at_10": 0.955, "kernel_ms": 77.5},
          {"result_expansion": 4.0, "epsilon": 0.093, "recall_at_10": 0.957, "kernel_ms": 79.2},
          {"result_expansion": 6.0, "epsilon": 0.085, "recall_at_10": 0.955, "kernel_ms": 76.5}]
    # 3.0 is within 3 % of the fastest (6.0): the tie goes to the default
    assert bench.pick_expansion(sw, 0.95)["result_expansion"] == 3.0
    # a clear winner is taken
    sw[3]["kernel_ms"] = 60.0
    assert bench.pick_expansion(sw, 0.95)["result_expansion"] == 6.0
    # one below the target is skipped while another reaches it
    sw[3]["recall_at_10"] = 0.94
    assert bench.pick_expansion(sw, 0.95)["result_expansion"] == 3.0


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float arrays a build-to-build comparison can load, the
    entries past each query's count zeroed, the same files from the same input."""
    ids = np.array([[7, 3, 9], [4, 1, 2]], np.uint32)
    dist = np.array([[0.5, 0.75, 9.0], [0.25, 1.5, 2.5]], np.float32)
    cnt = np.array([2, 3], np.int32)
    bench.dump_outputs(str(tmp_path / "a"), ids, dist, cnt)
    bench.dump_outputs(str(tmp_path / "b"), ids, dist, cnt)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("ids", "distances", "counts")}
    assert got["ids"].dtype == np.float64 and got["distances"].dtype == np.float32
    assert got["ids"].tolist() == [[7, 3, 0], [4, 1, 2]]
    assert got["distances"].tolist() == [[0.5, 0.75, 0.0], [0.25, 1.5, 2.5]]
    assert got["counts"].tolist() == [2, 3]
    assert not (tmp_path / "a" / "rows.npy").exists()
    for n in got:
        assert (tmp_path / "a" / (n + ".npy")).read_bytes() == (tmp_path / "b" / (n + ".npy")).read_bytes()


def test_dump_outputs_sample_is_bounded_and_fixed(tmp_path):
    """An output over the size limit is cut to a sample of the queries that is
    the same in every run (rows.npy names them) and fits the limit."""
    nq, k = 1000, 10
    ids = np.arange(nq * k, dtype=np.uint32).reshape(nq, k)
    dist = ids.astype(np.float32)
    cnt = np.full(nq, k, np.int32)
    limit = 20000
    bench.dump_outputs(str(tmp_path / "a"), ids, dist, cnt, max_bytes=limit)
    bench.dump_outputs(str(tmp_path / "b"), ids, dist, cnt, max_bytes=limit)
    rows = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy").astype(np.int64))
    assert 0 < len(rows) < nq and np.all(np.diff(rows) > 0)
    got = [np.load(tmp_path / "a" / (n + ".npy")) for n in ("rows", "ids", "distances", "counts")]
    assert sum(a.nbytes for a in got) <= limit
    assert np.array_equal(got[1], ids[rows]) and np.array_equal(got[2], dist[rows])


def test_plain_and_full_options_parse():
    """--full and --dump-outputs are options of the command itself (the dry
    run takes them like any other run)."""
    import json
    import os
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(bench._free_port()))
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "0",
                        "--full", "--dump-outputs", os.devnull], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2 and d["ms_per_step"] > 0


def test_traffic_entries_carry_clocked_passes():
    """The four timed lines' traffic.json entries (the ones bench.py attaches
    to C2, ANNG, qg and C3) hold both clocked counter passes: the SIMD issue
    figures and the texture address units' busy share, each a fraction of
    the GRBM-measured cycles."""
    import json
    import os
    t = json.load(open(os.path.join(os.path.dirname(bench.__file__), "profiles", "traffic.json")))
    clocked = [e for e in t["entries"] if "simd_issue" in e]
    assert len(clocked) == 4
    for e in clocked:
        ta = e["texture_address"]
        assert 0.0 < ta["ta_busy_frac"] < 1.0 and 0.0 < ta["vmem_per_cu_cycle"] < 1.0
        assert 0.0 < e["simd_issue"]["simd_valu_util"] <= e["simd_issue"]["simd_issue_util"]
