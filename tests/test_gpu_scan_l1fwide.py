"""The float L1 exact scan with lists of 17 .. 128 results on the byte-SAD
filter (ngt_amd/csrc/scan_l1f_wide.hip, opt-in by NGT_AMD_LINEAR_L1FWIDE)
against the reference's scan restated on the CPU: ids, distance bits and
counts, no tolerance anywhere, and the kernel that ran
(DeviceIndex.last_scan_kernel() == 10).  3001 rows: row 0 the dummy, a ragged
last 64-row tile; 160 queries: one full and one ragged 128-query block.  By
default the small table gets one tile per part (lists that never fill above
k = 63); NGT_AMD_SCAN_L1F_PARTS=2 gives parts of 24 and 23 tiles."""
import numpy as np
import pytest

import oracle_py as O
from ngt_amd.device import DeviceIndex, padded_dim

pytestmark = pytest.mark.gpu

N, NQ = 3001, 160
U32 = np.uint32


def oracle(rows, qs, k, radius=-1.0, valid=None):
    dim = rows.shape[1]
    pad = np.zeros((rows.shape[0], padded_dim(dim)), np.float32)
    pad[:, :dim] = rows
    qp = np.zeros((qs.shape[0], pad.shape[1]), np.float32)
    qp[:, :dim] = qs
    if valid is None:
        return O.linear_search_batch("l1", pad, qp, k, radius=radius, threads=8)
    oi, od, on = np.zeros((len(qp), k), U32), np.zeros((len(qp), k), np.float32), np.zeros(len(qp), U32)
    for q in range(len(qp)):
        i, d = O.linear_search("l1", pad, qp[q], k, valid=valid, radius=radius)
        on[q], oi[q, :len(i)], od[q, :len(i)] = len(i), i, d
    return oi, od, on


def check(monkeypatch, rows, qs, k, radius=-1.0, valid=None, kernel=10, metric="l1", otype="float", knob="1", parts=2):
    """knob None: NGT_AMD_LINEAR_L1FWIDE unset.  parts None: one tile per part."""
    if knob is None:
        monkeypatch.delenv("NGT_AMD_LINEAR_L1FWIDE", raising=False)
    else:
        monkeypatch.setenv("NGT_AMD_LINEAR_L1FWIDE", knob)
    if parts is not None:
        monkeypatch.setenv("NGT_AMD_SCAN_L1F_PARTS", str(parts))
    ix = DeviceIndex(metric, otype, rows.shape[1])
    try:
        ix.set_objects(rows, valid=valid)
        gi, gd, gn = ix.linear_search(qs.astype(np.float32), k=k, radius=radius)
        assert ix.last_scan_kernel() == kernel
    finally:
        ix.close()
    if metric != "l1":
        return None
    oi, od, on = oracle(rows, qs, k, radius, valid)
    assert np.array_equal(gn, on)
    live = np.arange(k)[None, :] < on[:, None]
    assert np.array_equal(gi[live], oi[live]), np.flatnonzero(((gi != oi) & live).any(1))[:8]
    assert np.array_equal(gd.view(U32)[live], od.view(U32)[live])
    return oi, od, on


def random_case(dim, seed=0, n=N):
    rng = np.random.default_rng(seed)
    rows = rng.random((n, dim), dtype=np.float32)
    rows[0] = 0
    rows[rng.integers(1, n, 40)] = rows[rng.integers(1, n, 40)]  # exact duplicates
    qs = rng.random((NQ, dim), dtype=np.float32)
    qs[:20] = rows[rng.integers(1, n, 20)]  # distance 0, ties by id
    return rows, qs


@pytest.mark.parametrize("parts", [None, 2])
@pytest.mark.parametrize("dim,k", [(8, 17), (100, 33), (128, 100), (200, 64), (256, 128)])
def test_random_rows(monkeypatch, dim, k, parts):
    """Every NC, two padded dimensions, one and two list keys per lane, both ends of k."""
    check(monkeypatch, *random_case(dim), k, parts=parts)


def test_small_integers_tie_in_float(monkeypatch):
    """Massive exact ties: ids decide, and a tile's survivors fill the slots several times."""
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 4, (N, 128)).astype(np.float32)
    check(monkeypatch, rows, rng.integers(0, 4, (NQ, 128)).astype(np.float32), 128)


@pytest.mark.parametrize("case", ["huge_rows", "shifted_queries", "nan_query"])
def test_outliers(monkeypatch, case):
    """huge_rows: two valid rows of +-1e18 and one with +inf -- a huge s, all
    codes equal, everything a candidate, the forced row ranked as the oracle
    ranks it.  shifted_queries: clamped query codes and a large e_q.
    nan_query: the largest T, every distance NaN, the ids in the order the
    reference's heap leaves them."""
    rows, qs = random_case(128, seed=3)
    if case == "huge_rows":
        rows[100], rows[2000], rows[1234, 7] = 1e18, -1e18, np.inf
    elif case == "shifted_queries":
        qs[40:80] += np.float32(5)
        qs[80:120] -= np.float32(5)
    else:
        qs[77, 5] = np.nan
    check(monkeypatch, rows, qs, 40)


def test_removed_rows_and_radius(monkeypatch):
    rows, qs = random_case(64, seed=4)
    valid = np.ones(N, np.uint8)
    valid[0] = 0
    valid[np.random.default_rng(5).choice(np.arange(1, N), 500, replace=False)] = 0
    # the median k-th distance: about half the lists are cut short
    r = float(np.median(oracle(rows, qs, 40, valid=valid)[1][:, 39]))
    for radius in (-1.0, r, 0.0):
        _, _, on = check(monkeypatch, rows, qs, 40, radius=radius, valid=valid)
        if radius == r:
            assert (on < 40).any() and (on == 40).any()


def test_short_table(monkeypatch):
    """k clamps to the 49 live rows; then a NaN query with rows 0, 1 and the last one removed."""
    rows, qs = random_case(32, seed=6, n=50)
    _, _, on = check(monkeypatch, rows, qs, 128)
    assert (on == 49).all()
    qs[[3, 77, 150], [0, 31, 8]] = np.nan
    valid = np.ones(50, np.uint8)
    valid[[0, 1, 49]] = 0
    check(monkeypatch, rows, qs, 128, valid=valid)


@pytest.mark.parametrize("dim,k,nq,knob,metric,kernel",
                         [(128, 17, NQ, None, "l1", 0), (128, 16, NQ, "1", "l1", 6), (128, 17, 31, "1", "l1", 0),
                          (272, 17, NQ, "1", "l1", 0), (128, 17, NQ, "1", "l2", 5)])
def test_routing(monkeypatch, dim, k, nq, knob, metric, kernel):
    """Without the knob, up to k = 16, below 32 queries, one chunk above Dp = 256, another metric:
    every call keeps its kernel, same results."""
    rows, qs = random_case(dim)
    check(monkeypatch, rows, qs[:nq], k, kernel=kernel, metric=metric, knob=knob)
