"""The uint8 L2 exact scan with lists of 17 .. 128 results on the int8 matrix
cores (ngt_amd/csrc/scan_u8_wide.hip, opt-in by NGT_AMD_LINEAR_U8WIDE) against
the reference's scan restated on the CPU: ids, distance bits and counts, and
the kernel that ran (DeviceIndex.last_scan_kernel() == 8).  3001 rows: row 0
the dummy, a partial 256-row tile, several parts; 160 queries: one full and
one ragged 128-query block."""
import numpy as np
import pytest

import oracle_py as O
from ngt_amd.device import DeviceIndex, padded_dim

pytestmark = pytest.mark.gpu

N, NQ = 3001, 160
U32 = np.uint32


def check(rows, qs, k, radius=-1.0, valid=None, kernel=8, metric="l2"):
    dim = rows.shape[1]
    pad = np.zeros((rows.shape[0], padded_dim(dim)), rows.dtype)
    pad[:, :dim] = rows
    qp = np.zeros((qs.shape[0], pad.shape[1]), rows.dtype)
    qp[:, :dim] = qs
    ix = DeviceIndex(metric, "uint8" if rows.dtype == np.uint8 else "float", dim)
    try:
        ix.set_objects(rows, valid=valid)
        gi, gd, gn = ix.linear_search(qs.astype(np.float32), k=k, radius=radius)
        assert ix.last_scan_kernel() == kernel
    finally:
        ix.close()
    if valid is None:
        oi, od, on = O.linear_search_batch(metric, pad, qp, k, radius=radius, threads=8)
    else:
        oi, od, on = np.zeros_like(gi), np.zeros_like(gd), np.zeros_like(gn)
        for q in range(len(qp)):
            i, d = O.linear_search(metric, pad, qp[q], k, valid=valid, radius=radius)
            on[q], oi[q, :len(i)], od[q, :len(i)] = len(i), i, d
    assert np.array_equal(gn, on)
    live = np.arange(k)[None, :] < on[:, None]
    assert np.array_equal(gi[live], oi[live]), np.flatnonzero(((gi != oi) & live).any(1))[:8]
    assert np.array_equal(gd.view(U32)[live], od.view(U32)[live])
    return oi, od, on


def random_case(dim, seed=0, n=N):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    rows[rng.integers(1, n, 40)] = rows[rng.integers(1, n, 40)]  # exact duplicates
    qs = rng.integers(0, 256, (NQ, dim)).astype(np.uint8)
    qs[:20] = rows[rng.integers(1, n, 20)]  # distance 0, ties by id
    return rows, qs


def sums(rows, qs):
    """int64 sums of squared differences [nq, n]."""
    r, q = rows.astype(np.int64), qs.astype(np.int64)
    return (q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2 * q @ r.T


@pytest.mark.parametrize("parts", [None, "2"])
@pytest.mark.parametrize("dim,k", [(8, 17), (100, 33), (128, 100), (256, 128), (768, 20)])
def test_random_bytes(monkeypatch, dim, k, parts):
    """The padded dimension, both ends of k, more than one list word per lane,
    64 and (dim 768) 32 pending slots; parts of one tile and, with the cap,
    parts of six."""
    monkeypatch.setenv("NGT_AMD_LINEAR_U8WIDE", "1")
    if parts is not None:
        monkeypatch.setenv("NGT_AMD_SCAN_WIDE_PARTS", parts)
    check(*random_case(dim), k)


def test_sums_above_two_to_the_24(monkeypatch):
    """Every survivor's distance comes from the stored bytes on one lane (and
    long rows leave 16 pending slots)."""
    monkeypatch.setenv("NGT_AMD_LINEAR_U8WIDE", "1")
    rng = np.random.default_rng(2)
    rows = rng.integers(192, 256, (N, 960)).astype(np.uint8)
    qs = rng.integers(0, 64, (64, 960)).astype(np.uint8)
    _, od, _ = check(rows, qs, 20)
    assert (od[:, 19].astype(np.float64) ** 2 > 1 << 24).all()


def test_float_ties_of_distinct_sums(monkeypatch):
    monkeypatch.setenv("NGT_AMD_LINEAR_U8WIDE", "1")
    rng = np.random.default_rng(1)
    rows, qs = np.zeros((N, 128), np.uint8), np.full((NQ, 128), 255, np.uint8)
    rows[:, -8:] = rng.integers(0, 4, (N, 8))
    qs[:, -8:] = rng.integers(0, 4, (NQ, 8))
    oi, _, _ = check(rows, qs, 20)
    S = sums(rows, qs)
    S[:, 0] = 1 << 40  # the dummy row
    # the fixture still has queries that a ranking by (S, id) gets wrong
    by_sum = np.lexsort((np.broadcast_to(np.arange(N), S.shape), S))[:, :20]
    assert (by_sum != oi).any(1).sum() >= 1


def test_identical_rows(monkeypatch):
    """Every tile overflows the pending slots; the lowest live ids win."""
    monkeypatch.setenv("NGT_AMD_LINEAR_U8WIDE", "1")
    monkeypatch.setenv("NGT_AMD_SCAN_WIDE_PARTS", "2")
    rows, qs = random_case(128, seed=3)
    rows[:] = rows[1]
    oi, _, _ = check(rows, qs, 40)
    assert (oi == np.arange(1, 41)).all()


@pytest.mark.parametrize("radius", [-1.0, None, 0.0])
def test_removed_rows_and_radius(monkeypatch, radius):
    monkeypatch.setenv("NGT_AMD_LINEAR_U8WIDE", "1")
    rows, qs = random_case(64, seed=4)
    valid = np.ones(N, np.uint8)
    valid[0] = 0
    valid[np.random.default_rng(5).choice(np.arange(1, N), 500, replace=False)] = 0
    if radius is None:  # the median k-th distance: cuts some lists short, others are full
        radius = float(np.median([O.linear_search("l2", rows, q, 20, valid=valid)[1][19] for q in qs]))
    _, _, on = check(rows, qs, 20, radius=radius, valid=valid)
    if radius > 0.0:
        assert (on < 20).any() and (on == 20).any()


def test_short_table(monkeypatch):
    monkeypatch.setenv("NGT_AMD_LINEAR_U8WIDE", "1")
    rows, qs = random_case(128, seed=6, n=100)
    _, _, on = check(rows, qs, 128)
    assert (on == 99).all()


@pytest.mark.parametrize("metric,dtype,k,nq,knob,kernel", [
    ("l2", np.uint8, 17, NQ, "1", 8), ("l2", np.uint8, 128, NQ, "1", 8), ("l2", np.uint8, 16, NQ, "1", 3),
    ("l2", np.uint8, 129, NQ, "1", 0), ("l2", np.uint8, 17, 31, "1", 0), ("cosine", np.uint8, 17, NQ, "1", 7),
    ("l2", np.float32, 17, NQ, "1", 5), ("l2", np.uint8, 17, NQ, "0", 0), ("l2", np.uint8, 17, NQ, None, 0)])
def test_routing(monkeypatch, metric, dtype, k, nq, knob, kernel):
    """The new kernel answers only with the knob on, for 17 .. 128 results and
    at least 32 queries; every other shape keeps its kernel."""
    if knob is not None:
        monkeypatch.setenv("NGT_AMD_LINEAR_U8WIDE", knob)
    rows, qs = random_case(128)
    check(rows.astype(dtype), qs[:nq].astype(dtype), k, kernel=kernel, metric=metric)
