"""The uint8 L1 / Hamming exact scan with lists of 17 .. 128 results and the
uint8 Jaccard exact scan with lists of 1 .. 128 (ngt_amd/csrc/scan_bytes_wide.hip,
opt-in by NGT_AMD_LINEAR_BYTESWIDE) against the reference's scan restated on
the CPU: ids, distance bits and counts, and the kernel that ran
(DeviceIndex.last_scan_kernel() == 9).  3001 rows: row 0 the dummy, a ragged
last 64-row tile, several parts (of one tile, and with NGT_AMD_SCAN_WIDE_PARTS
of ten); 160 queries: one full and one ragged 128-query block."""
import numpy as np
import pytest

import oracle_py as O
from ngt_amd.device import DeviceIndex, padded_dim

pytestmark = pytest.mark.gpu

N, NQ = 3001, 160
U32 = np.uint32
METRICS = ["l1", "hamming", "jaccard"]


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


def check(metric, rows, qs, k, radius=-1.0, valid=None, kernel=9):
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


def case(dim, seed=0, n=N, density=None):
    """Random bytes with exact duplicate rows and 20 queries copied from rows;
    with a density, binary rows and queries with that share of bits set, no
    all-zero row, five all-zero queries."""
    rng = np.random.default_rng(seed)
    if density is None:
        rows = rng.integers(0, 256, (n, dim)).astype(np.uint8)
        qs = rng.integers(0, 256, (NQ, dim)).astype(np.uint8)
    else:
        rows = np.packbits(rng.random((n, dim * 8)) < density, axis=1)
        rows[~rows.any(1), 0] = 1
        qs = np.packbits(rng.random((NQ, dim * 8)) < density, axis=1)
    rows[rng.integers(1, n, 40)] = rows[rng.integers(1, n, 40)]  # exact duplicates
    qs[:20] = rows[rng.integers(1, n, 20)]  # distance 0, ties by id
    if density is not None:
        qs[20:25] = 0
    return rows, qs


@pytest.mark.parametrize("parts", [None, "5"])
@pytest.mark.parametrize("metric,dim,k", [(m, d, k) for m in METRICS for d, k in
                                          [(8, 17), (100, 33), (128, 100), (200, 64), (256, 128)]] +
                         [("jaccard", 16, 1), ("jaccard", 128, 10)])
def test_random_bytes(monkeypatch, metric, dim, k, parts):
    """Every row length in registers (1, 8 and 16 chunks, two of them padded),
    both ends of k, one and two list keys per lane; dim 8: heavy ties by id."""
    monkeypatch.setenv("NGT_AMD_LINEAR_BYTESWIDE", "1")
    if parts is not None:
        monkeypatch.setenv("NGT_AMD_SCAN_WIDE_PARTS", parts)
    check(metric, *case(dim), k)


def test_sparse_binary_rows(monkeypatch):
    """Many pairs share no bit: distance 1, ranked by id; all-zero queries
    rank the whole table by id."""
    monkeypatch.setenv("NGT_AMD_LINEAR_BYTESWIDE", "1")
    monkeypatch.setenv("NGT_AMD_SCAN_WIDE_PARTS", "5")
    _, od, _ = check("jaccard", *case(128, seed=2, density=0.05), 100)
    assert (od[20:25] == 1.0).all()


@pytest.mark.parametrize("metric", METRICS)
def test_all_rows_equal(monkeypatch, metric):
    """Every tile fills the pending slots four times over; the lowest ids win."""
    monkeypatch.setenv("NGT_AMD_LINEAR_BYTESWIDE", "1")
    monkeypatch.setenv("NGT_AMD_SCAN_WIDE_PARTS", "5")
    rng = np.random.default_rng(1)
    rows = np.repeat(rng.integers(0, 256, (1, 32)), N, 0).astype(np.uint8)
    oi, _, _ = check(metric, rows, rng.integers(0, 256, (NQ, 32)).astype(np.uint8), 128)
    assert np.array_equal(oi, np.broadcast_to(np.arange(1, 129, dtype=U32), oi.shape))


@pytest.mark.parametrize("metric", METRICS)
def test_removed_rows_and_radius(monkeypatch, metric):
    monkeypatch.setenv("NGT_AMD_LINEAR_BYTESWIDE", "1")
    monkeypatch.setenv("NGT_AMD_SCAN_WIDE_PARTS", "5")
    rows, qs = case(64, seed=4)
    valid = np.ones(N, np.uint8)
    valid[0] = 0
    valid[np.random.default_rng(5).choice(np.arange(1, N), 500, replace=False)] = 0
    _, od, _ = check(metric, rows, qs, 40, valid=valid)
    # the median k-th distance: some lists are cut short, others are full
    _, _, on = check(metric, rows, qs, 40, radius=float(np.median(od[:, 39])), valid=valid)
    assert (on < 40).any() and (on == 40).any()


@pytest.mark.parametrize("metric", METRICS)
def test_table_shorter_than_the_list(monkeypatch, metric):
    monkeypatch.setenv("NGT_AMD_LINEAR_BYTESWIDE", "1")
    _, _, on = check(metric, *case(128, seed=6, n=50), 128)
    assert (on == 49).all()


@pytest.mark.parametrize("metric,dim,k,nq,knob,zero,kernel", [
    ("jaccard", 128, 10, NQ, None, False, 0), ("l1", 128, 17, NQ, None, False, 0), ("l1", 128, 16, NQ, "1", False, 4),
    ("hamming", 128, 17, 31, "1", False, 0), ("jaccard", 128, 10, 31, "1", False, 0),
    ("jaccard", 272, 10, NQ, "1", False, 0), ("l1", 272, 17, NQ, "1", False, 0),
    ("jaccard", 128, 10, NQ, "1", True, 0)])
def test_routing(monkeypatch, metric, dim, k, nq, knob, zero, kernel):
    """Without the knob, below the batch size, one chunk above the row bound
    and for a Jaccard table with an all-zero live row (and an all-zero query)
    the quad-per-row kernel answers, L1 with 16 results keeps its kernel --
    with the same results each time.  The all-zero row is row 1: the
    reference's heap then holds the NaN of (all-zero query, all-zero row) at
    its top and pops it first, as the quad-per-row kernel's keys rank it last;
    from a later row the NaN stays in the heap, which that kernel never
    followed."""
    if knob is not None:
        monkeypatch.setenv("NGT_AMD_LINEAR_BYTESWIDE", knob)
    rows, qs = case(dim)
    if zero:
        rows[1] = 0
        qs[30] = 0
    check(metric, rows, qs[:nq], k, kernel=kernel)
