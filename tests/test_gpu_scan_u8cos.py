"""The uint8 Cosine / Angle exact scan on the int8 matrix cores
(ngt_amd/csrc/scan_u8cos.hip) against the reference's scan restated on the
CPU: ids, distance bits and counts, and the kernel that ran
(DeviceIndex.last_scan_kernel() == 7).  3001 rows: row 0 the dummy, a partial
256-row tile, several parts; 160 queries: one full and one ragged 128-query
block.  Every case runs both metrics."""
import numpy as np
import pytest

import oracle_py as O
from ngt_amd.device import DeviceIndex, padded_dim

pytestmark = pytest.mark.gpu

N, NQ = 3001, 160
U32 = np.uint32
METRICS = ("cosine", "angle")


def device(metric, rows, qs, k, radius=-1.0, valid=None, kernel=7, otype="uint8"):
    ix = DeviceIndex(metric, otype, rows.shape[1])
    try:
        ix.set_objects(rows, valid=valid)
        out = ix.linear_search(qs.astype(np.float32), k=k, radius=radius)
        assert ix.last_scan_kernel() == kernel
    finally:
        ix.close()
    return out


def check(metric, rows, qs, k, radius=-1.0, valid=None, kernel=7):
    dim = rows.shape[1]
    pad = np.zeros((rows.shape[0], padded_dim(dim)), np.uint8)
    pad[:, :dim] = rows
    qp = np.zeros((qs.shape[0], pad.shape[1]), np.uint8)
    qp[:, :dim] = qs
    gi, gd, gn = device(metric, rows, qs, k, radius, valid, kernel)
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


def random_case(dim, seed=0, n=N, nq=NQ):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    rows[rng.integers(1, n, 40)] = rows[rng.integers(1, n, 40)]  # exact duplicates
    qs = rng.integers(0, 256, (nq, dim)).astype(np.uint8)
    qs[:20] = rows[rng.integers(1, n, 20)]  # parallel to a row, ties by id
    return rows, qs


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim,k,nq", [(8, 10, NQ), (100, 1, NQ), (128, 16, NQ), (200, 33, NQ), (256, 128, NQ),
                                      (960, 10, 64)])
def test_random_bytes(metric, dim, k, nq):
    """The padded dimension, both ends of k, more than one list word per lane,
    long rows (16 pending slots) and s > 2^24."""
    check(metric, *random_case(dim, nq=nq), k)


def near_copies(base, n, rng):
    rows = np.repeat(base[None, :], n, 0)
    rows[:, -8:] = rng.integers(0, 4, (n, 8))
    return rows.astype(np.uint8)


@pytest.mark.parametrize("metric", METRICS)
def test_float_ties_of_distinct_cosines(metric):
    rng = np.random.default_rng(1)
    rows = near_copies(rng.integers(0, 256, 128), N, rng)
    qs = near_copies(rng.integers(0, 256, 128), NQ, rng)
    oi, _, _ = check(metric, rows, qs, 10)
    r, q = rows.astype(np.int64), qs.astype(np.int64)
    c = (q @ r.T) / np.sqrt(((q * q).sum(1)[:, None] * (r * r).sum(1)[None, :]).astype(np.float64))
    c[:, 0] = -1.0  # the dummy row
    # the fixture still has queries that a ranking by (c, id) gets wrong
    by_c = np.lexsort((np.broadcast_to(np.arange(N), c.shape), -c))[:, :10]
    assert (by_c != oi).any(1).sum() >= 1


@pytest.mark.parametrize("metric", METRICS)
def test_parallel_rows(metric):
    """Rows equal to the query and to twice the query: c = 1, distance 0 under
    both metrics, ties by id."""
    rows, _ = random_case(128, seed=3)
    rng = np.random.default_rng(3)
    qs = rng.integers(0, 128, (NQ, 128)).astype(np.uint8)
    at = rng.choice(np.arange(1, N), 2 * NQ, replace=False)
    rows[at[:NQ]] = qs
    rows[at[NQ:]] = 2 * qs
    _, od, _ = check(metric, rows, qs, 10)
    assert (od[:, :2] <= 0.0).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("radius", [-1.0, None, 0.0])
def test_removed_rows_and_radius(metric, radius):
    rows, qs = random_case(64, seed=4)
    valid = np.ones(N, np.uint8)
    valid[0] = 0
    valid[np.random.default_rng(5).choice(np.arange(1, N), 500, replace=False)] = 0
    if radius is None:  # the median k-th distance: cuts some lists short, others are full
        pad = np.zeros((N, padded_dim(64)), np.uint8)
        pad[:, :64] = rows
        kth = [O.linear_search(metric, pad, np.pad(q, (0, pad.shape[1] - 64)), 10, valid=valid)[1][9] for q in qs]
        radius = float(np.median(kth))
    _, _, on = check(metric, rows, qs, 10, radius=radius, valid=valid)
    if radius > 0.0:
        assert (on < 10).any() and (on == 10).any()


@pytest.mark.parametrize("metric", METRICS)
def test_short_table(metric):
    rows, qs = random_case(128, seed=6, n=100)
    _, _, on = check(metric, rows, qs, 128)
    assert (on == 99).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,k", [(N, 10), (100, 128)])
def test_nan_conventions(monkeypatch, metric, n, k):
    """A row of zeros and a query of zeros have NaN distances: what the
    quad-per-row kernel returns for them.  The row of zeros is the table's
    last: it is not among the first k of any slice of the quad kernel, whose
    k-th distance would otherwise turn NaN and stop that slice."""
    rows, qs = random_case(128, seed=7, n=n)
    rows[n - 1] = 0
    qs[5] = 0
    gi, gd, gn = device(metric, rows, qs, k)
    monkeypatch.setenv("NGT_AMD_LINEAR_U8COS", "0")
    qi, qd, qn = device(metric, rows, qs, k, kernel=0)
    live = np.arange(k)[None, :] < qn[:, None]
    assert np.array_equal(gn, qn) and np.array_equal(gi[live], qi[live])
    assert np.array_equal(gd.view(U32)[live], qd.view(U32)[live])
    assert np.isnan(gd[5, :gn[5]]).all()
    if n == 100:
        assert (gi[:, 98] == 99).all() and np.isnan(gd[:, 98]).all()


@pytest.mark.parametrize("metric,otype,k,nq,knob,kernel", [
    ("cosine", "uint8", 16, NQ, None, 7), ("angle", "uint8", 17, NQ, None, 7), ("cosine", "uint8", 128, NQ, None, 7),
    ("angle", "uint8", 16, 32, None, 7), ("cosine", "uint8", 129, NQ, None, 0), ("angle", "uint8", 10, 31, None, 0),
    ("cosine", "uint8", 10, NQ, "0", 0), ("l2", "uint8", 10, NQ, None, 3), ("jaccard", "uint8", 10, NQ, None, 0),
    ("cosine", "float", 10, NQ, None, 2)])
def test_routing(monkeypatch, metric, otype, k, nq, knob, kernel):
    """Beyond the list length, below the batch size or with the knob off the
    quad-per-row kernel answers; the other scans keep their kernels."""
    if knob is not None:
        monkeypatch.setenv("NGT_AMD_LINEAR_U8COS", knob)
    rows, qs = random_case(128)
    if otype == "float":
        device(metric, rows.astype(np.float32), qs[:nq], k, kernel=kernel, otype=otype)
    elif metric in METRICS:
        check(metric, rows, qs[:nq], k, kernel=kernel)
    else:
        device(metric, rows, qs[:nq], k, kernel=kernel)
