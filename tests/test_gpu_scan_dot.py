"""The matrix-core filtered exact scans (scan_mfma_dot.hip: k <= 16, kernel 2;
scan_mfma_wide.hip: 17 <= k <= 128, kernel 5) for float Angle, Normalized
Angle, Normalized Cosine and Normalized L2 against the reference's scan
restated on the CPU: ids, distance bits and counts, no tolerance anywhere, and
the kernel that ran.  The table, check() and oracle() are test_gpu_scan_wide's:
2,881 rows (11 full tiles and one of 65 rows), 160 queries; the wide cases run
with one part (bootstrap tile + 11 steady tiles) and with the default split."""
import ctypes

import numpy as np
import pytest

import oracle_py as O
from test_gpu_scan_wide import N, NQ, check, oracle

pytestmark = pytest.mark.gpu

NORMALIZED = ["normalized_cosine", "normalized_angle", "normalized_l2"]
METRICS = NORMALIZED + ["angle"]


def unit(a):
    n = np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True)
    return (a / np.where(n > 0, n, 1)).astype(np.float32)


def prepared(metric, qs):
    """The queries as the library prepares them: the reference's normalization under the normalized metrics."""
    out = np.ascontiguousarray(qs, np.float32).copy()
    for v in out if metric in NORMALIZED else ():
        assert O.lib().ngto_normalize_f32(v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(v)) == 0
    return out


def run(monkeypatch, metric, rows, qs, k, kernel=None, **kw):
    """One part and the default split for the wide kernel; the LDS-list kernel has one form."""
    expect = oracle(metric, rows, prepared(metric, qs), k, kw.get("radius", -1.0), kw.get("valid"))
    for parts in ((1, None) if k > 16 and kernel is None else (None,)):
        check(monkeypatch, metric, rows, qs, k, parts, kernel=(5 if k > 16 else 2) if kernel is None else kernel,
              expect=expect, **kw)
    return expect


def random_case(metric, dim, seed=0):
    """Rows on the unit sphere (raw for Angle), 40 exact duplicates, 20 queries equal to stored rows."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((N, dim), np.float32)
    rows[1:] = rng.random((N - 1, dim), dtype=np.float32) - np.float32(0.5)
    qs = rng.random((NQ, dim), dtype=np.float32) - np.float32(0.5)
    if metric != "angle":
        rows, qs = unit(rows), unit(qs)
    rows[rng.integers(1, N, 40)] = rows[rng.integers(1, N, 40)]
    qs[:20] = rows[rng.integers(1, N, 20)]
    return rows, qs


@pytest.mark.parametrize("dim,k", [(8, 10), (100, 16), (128, 17), (128, 100), (960, 64)])
@pytest.mark.parametrize("metric", METRICS)
def test_random_rows(monkeypatch, metric, dim, k):
    run(monkeypatch, metric, *random_case(metric, dim), k)


@pytest.mark.parametrize("k", [16, 100])
@pytest.mark.parametrize("metric", METRICS)
def test_cluster_near_one(monkeypatch, metric, k):
    """Every dot product within a few thousand ulps of 1: the steep end of acos
    and of sqrt(2 - 2 dot), many equal float distances of distinct dot products."""
    rng = np.random.default_rng(7)
    q0 = unit(rng.standard_normal((1, 128)))
    rows = unit(q0 + np.float32(1e-4) * rng.standard_normal((N, 128)).astype(np.float32))
    rows[0] = 0
    qs = unit(q0 + np.float32(1e-4) * rng.standard_normal((NQ, 128)).astype(np.float32))
    run(monkeypatch, metric, rows, qs, k)


@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("metric", NORMALIZED)
def test_unnormalized_rows(monkeypatch, metric, k):
    """Row norms in [0.2, 3] under the normalized metrics (the library normalizes
    the queries, never the rows): dot > 1 clamps to distance 0 in id order,
    dot < -1 to pi for the angle, and Xmax dwarfs a unit row."""
    rng = np.random.default_rng(8)
    rows = unit(rng.standard_normal((N, 8))) * rng.uniform(0.2, 3, (N, 1)).astype(np.float32)
    rows[0] = 0
    qs = unit(rng.standard_normal((NQ, 8))) * rng.uniform(0.2, 3, (NQ, 1)).astype(np.float32)
    dots = prepared(metric, qs).astype(np.float64) @ rows.astype(np.float64).T
    assert ((dots > 1).sum(1) > k).sum() > NQ // 4 and (dots < -1).any()
    run(monkeypatch, metric, rows, qs, k)


@pytest.mark.parametrize("metric,k", [("normalized_cosine", 40), ("normalized_cosine", 12), ("angle", 40), ("angle", 12)])
def test_removed_rows_and_radius(monkeypatch, metric, k):
    rows, qs = random_case(metric, 64, seed=4)
    rng = np.random.default_rng(5)
    valid = np.ones(N, np.uint8)
    valid[0] = 0
    valid[rng.choice(np.arange(1, N), 500, replace=False)] = 0
    valid[rng.permutation(np.arange(1, 256))[10:]] = 0  # the first tile: fewer than k live rows
    free = run(monkeypatch, metric, rows, qs, k, valid=valid)
    r = float(np.median(free[1][:, k - 1]))
    run(monkeypatch, metric, rows, qs, k, valid=valid, radius=0.0)
    on = run(monkeypatch, metric, rows, qs, k, valid=valid, radius=r)[2]
    assert (on < k).any() and (on == k).any()


@pytest.mark.parametrize("k", [16, 100])
def test_non_finite_and_zero_rows(monkeypatch, k):
    """A row with an inf and an all-zero row under Angle: both are forced past
    the filter, and the comparator's NaN is ranked as the oracle ranks it."""
    rows, qs = random_case("angle", 40, seed=9)
    rows[300, 3] = np.inf
    rows[1500] = 0
    run(monkeypatch, "angle", rows, qs, k)


@pytest.mark.parametrize("metric,k,nq,knob,kernel",
                         [(m, 16, NQ, None, 2) for m in METRICS] + [(m, 17, NQ, None, 5) for m in METRICS] +
                         [("normalized_cosine", 129, NQ, None, 0), ("normalized_angle", 100, 31, None, 0),
                          ("normalized_l2", 100, NQ, "0", 0), ("angle", 10, NQ, "0", 0), ("l1", 17, NQ, None, 0)])
def test_routing(monkeypatch, metric, k, nq, knob, kernel):
    if knob is not None:
        monkeypatch.setenv("NGT_AMD_LINEAR_DOT", knob)
    rows, qs = random_case(metric, 128)
    run(monkeypatch, metric, rows, qs[:nq], k, kernel=kernel)
