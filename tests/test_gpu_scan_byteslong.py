"""The uint8 L1 / Hamming exact scan of rows of 272 .. 1024 padded bytes
(ngt_amd/csrc/scan_bytes_long.hip, behind NGT_AMD_LINEAR_BYTESLONG) against
the reference's scan restated on the CPU: ids, distance bits and counts, and
the kernel that ran (DeviceIndex.last_scan_kernel() == 11).  3001 rows: row 0
the dummy, a ragged last 64-row tile, five parts of several tiles
(NGT_AMD_SCAN_WIDE_PARTS) or one part per tile; 160 queries: two full and one
ragged 64-query block."""
import numpy as np
import pytest

import oracle_py as O
from ngt_amd.device import DeviceIndex, padded_dim

pytestmark = pytest.mark.gpu

N, NQ = 3001, 160
U32 = np.uint32
METRICS = ["l1", "hamming"]


def oracle(metric, rows, qs, k, radius=-1.0, valid=None):
    dim = rows.shape[1]
    pad = np.zeros((rows.shape[0], padded_dim(dim)), np.uint8)
    pad[:, :dim] = rows
    qp = np.zeros((qs.shape[0], pad.shape[1]), np.uint8)
    qp[:, :dim] = qs
    if valid is None:
        return O.linear_search_batch(metric, pad, qp, k, radius=radius, threads=8)
    oi, od, on = np.zeros((len(qp), k), U32), np.zeros((len(qp), k), np.float32), np.zeros(len(qp), U32)
    for q in range(len(qp)):
        i, d = O.linear_search(metric, pad, qp[q], k, valid=valid, radius=radius)
        on[q], oi[q, :len(i)], od[q, :len(i)] = len(i), i, d
    return oi, od, on


def check(metric, rows, qs, k, radius=-1.0, valid=None, kernel=11):
    ix = DeviceIndex(metric, "uint8", rows.shape[1])
    try:
        ix.set_objects(rows, valid=valid)
        gi, gd, gn = ix.linear_search(qs.astype(np.float32), k=k, radius=radius)
        assert ix.last_scan_kernel() == kernel
    finally:
        ix.close()
    oi, od, on = oracle(metric, rows, qs, k, radius, valid)
    assert np.array_equal(gn, on)
    live = np.arange(k)[None, :] < on[:, None]
    assert np.array_equal(gi[live], oi[live]), np.flatnonzero(((gi != oi) & live).any(1))[:8]
    assert np.array_equal(gd.view(U32)[live], od.view(U32)[live])
    return oi, od, on


def random_case(dim, seed=0):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (N, dim)).astype(np.uint8)
    rows[rng.integers(1, N, 40)] = rows[rng.integers(1, N, 40)]  # exact duplicates
    qs = rng.integers(0, 256, (NQ, dim)).astype(np.uint8)
    qs[:20] = rows[rng.integers(1, N, 20)]  # distance 0, ties by id
    return rows, qs


@pytest.fixture
def knobs(monkeypatch):
    monkeypatch.setenv("NGT_AMD_LINEAR_BYTESLONG", "1")
    monkeypatch.setenv("NGT_AMD_SCAN_WIDE_PARTS", "5")
    return monkeypatch


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim,k", [(272, 10), (500, 1), (512, 16), (1000, 7), (1024, 10)])
def test_random_bytes(knobs, metric, dim, k):
    """One chunk above the old bound with a ragged last piece, two dimensions
    that are no multiple of 16, the last shape served."""
    check(metric, *random_case(dim), k)


@pytest.mark.parametrize("metric,top", [("l1", 255 * 1024), ("hamming", 8 * 1024)])
def test_largest_sums(knobs, metric, top):
    """The largest sum an accumulator and the first-tile selection must hold:
    all but a few rows tie at it and are ranked by id."""
    rng = np.random.default_rng(2)
    rows = np.zeros((N, 1024), np.uint8)
    some = rng.choice(np.arange(1, N), 5, replace=False)
    rows[some] = rng.integers(0, 256, (5, 1024))
    oi, od, _ = check(metric, rows, np.full((NQ, 1024), 255, np.uint8), 16)
    assert (od[:, 5:] == top).all() and (od[:, :5] < top).all()
    assert np.array_equal(oi[0, 5:], np.setdiff1d(np.arange(1, 30), some)[:11])


@pytest.mark.parametrize("metric", METRICS)
def test_all_rows_equal(knobs, metric):
    rng = np.random.default_rng(1)
    rows = np.repeat(rng.integers(0, 256, (1, 320)), N, 0).astype(np.uint8)
    oi, _, _ = check(metric, rows, rng.integers(0, 256, (NQ, 320)).astype(np.uint8), 16)
    assert np.array_equal(oi, np.broadcast_to(np.arange(1, 17, dtype=U32), oi.shape))


@pytest.mark.parametrize("metric", METRICS)
def test_removed_rows_and_radius(knobs, metric):
    rows, qs = random_case(512, seed=4)
    valid = np.ones(N, np.uint8)
    valid[0] = 0
    valid[np.random.default_rng(5).choice(np.arange(1, N), 500, replace=False)] = 0
    # the median k-th distance: about half the lists are cut short
    r = float(np.median(oracle(metric, rows, qs, 10, valid=valid)[1][:, 9]))
    for radius in (-1.0, r, 0.0):
        _, _, on = check(metric, rows, qs, 10, radius=radius, valid=valid)
        if radius == r:
            assert (on < 10).any() and (on == 10).any()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim,k,nq,knob,kernel", [(512, 10, NQ, None, 0), (512, 10, NQ, "0", 0), (1040, 10, NQ, "1", 0),
                                                  (512, 17, NQ, "1", 0), (512, 10, 31, "1", 0), (256, 10, NQ, "1", 4),
                                                  (512, 16, 32, "1", 11)])
def test_routing(monkeypatch, metric, dim, k, nq, knob, kernel):
    """Without the knob, beyond the row bound or the list length and below the
    batch size the quad-per-row kernel answers, a 256-byte row keeps kernel 4:
    the same results everywhere.  One part per tile here."""
    if knob is not None:
        monkeypatch.setenv("NGT_AMD_LINEAR_BYTESLONG", knob)
    rows, qs = random_case(dim)
    check(metric, rows, qs[:nq], k, kernel=kernel)
