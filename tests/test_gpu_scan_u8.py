"""The uint8 L2 exact scan on the int8 matrix cores (ngt_amd/csrc/scan_u8.hip)
against the reference's scan restated on the CPU: ids, distance bits and
counts, and the kernel that ran (DeviceIndex.last_scan_kernel() == 3).
3001 rows: row 0 the dummy, a partial 256-row tile, several parts; 160
queries: one full and one ragged 128-query block."""
import numpy as np
import pytest

import oracle_py as O
from ngt_amd.device import DeviceIndex, padded_dim

pytestmark = pytest.mark.gpu

N, NQ = 3001, 160
U32 = np.uint32


def make_rows(fill, tail, rng, hi, n=N, bump=None):
    """n rows of `fill` with the last `tail` bytes drawn from [0, hi) (+ bump[row])."""
    rows = np.full((n, fill[1]), fill[0], np.int64)
    rows[:, fill[1] - tail:] = rng.integers(0, hi, (n, tail))
    if bump is not None:
        rows[:, fill[1] - tail:] += bump[:, None]
    return rows.astype(np.uint8)


def check(rows, qs, k, radius=-1.0, valid=None, kernel=3):
    dim = rows.shape[1]
    pad = np.zeros((rows.shape[0], padded_dim(dim)), np.uint8)
    pad[:, :dim] = rows
    qp = np.zeros((qs.shape[0], pad.shape[1]), np.uint8)
    qp[:, :dim] = qs
    ix = DeviceIndex("l2", "uint8", dim)
    try:
        ix.set_objects(rows, valid=valid)
        gi, gd, gn = ix.linear_search(qs.astype(np.float32), k=k, radius=radius)
        assert ix.last_scan_kernel() == kernel
    finally:
        ix.close()
    if valid is None:
        oi, od, on = O.linear_search_batch("l2", pad, qp, k, radius=radius, threads=8)
    else:
        oi, od, on = np.zeros_like(gi), np.zeros_like(gd), np.zeros_like(gn)
        for q in range(len(qp)):
            i, d = O.linear_search("l2", pad, qp[q], k, valid=valid, radius=radius)
            on[q], oi[q, :len(i)], od[q, :len(i)] = len(i), i, d
    assert np.array_equal(gn, on)
    live = np.arange(k)[None, :] < on[:, None]
    assert np.array_equal(gi[live], oi[live]), np.flatnonzero(((gi != oi) & live).any(1))[:8]
    assert np.array_equal(gd.view(U32)[live], od.view(U32)[live])
    return oi, on


def random_case(dim, seed=0):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (N, dim)).astype(np.uint8)
    rows[rng.integers(1, N, 40)] = rows[rng.integers(1, N, 40)]  # exact duplicates
    qs = rng.integers(0, 256, (NQ, dim)).astype(np.uint8)
    qs[:20] = rows[rng.integers(1, N, 20)]  # distance 0, ties by id
    return rows, qs


@pytest.mark.parametrize("dim,k", [(8, 10), (100, 1), (128, 16), (200, 7), (256, 10)])
def test_random_bytes(dim, k):
    check(*random_case(dim), k)


def sums(rows, qs):
    """int64 sums of squared differences [nq, n]."""
    r, q = rows.astype(np.int64), qs.astype(np.int64)
    return (q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2 * q @ r.T


def test_float_ties_of_distinct_sums():
    rng = np.random.default_rng(1)
    rows = make_rows((0, 128), 8, rng, 4)
    qs = make_rows((255, 128), 8, rng, 4, n=NQ)
    oi, _ = check(rows, qs, 10)
    S = sums(rows, qs)
    S[:, 0] = 1 << 40  # the dummy row
    assert S[:, 1:].min() >= 7803000 and S[:, 1:].max() <= 7803064
    # the fixture still has queries that a ranking by (S, id) gets wrong
    by_sum = np.lexsort((np.broadcast_to(np.arange(N), S.shape), S))[:, :10]
    assert (by_sum != oi).any(1).sum() >= 1


@pytest.mark.parametrize("dim,nq", [(288, NQ), (960, 64)])
def test_sums_around_two_to_the_24(dim, nq):
    rng = np.random.default_rng(2)
    if dim == 288:
        rows = make_rows((0, 288), 30, rng, 16)
        qs = make_rows((255, 288), 30, rng, 16, n=nq, bump=np.arange(nq) % 8)
    else:  # every sum far above 2^24: all recomputed, the rejection rule never fires
        rows = rng.integers(0, 16, (N, dim)).astype(np.uint8)
        qs = rng.integers(240, 256, (nq, dim)).astype(np.uint8)
    oi, _ = check(rows, qs, 10)
    top = np.take_along_axis(sums(rows, qs), oi.astype(np.int64), 1)
    below, above = (top < 1 << 24).all(1), (top >= 1 << 24).all(1)
    if dim == 288:
        assert below.any() and above.any() and (~below & ~above).any()
    else:
        assert above.all()


@pytest.mark.parametrize("radius", [-1.0, 650.0, 0.0])
def test_removed_rows_and_radius(radius):
    rows, qs = random_case(64, seed=4)
    valid = np.ones(N, np.uint8)
    valid[0] = 0
    valid[np.random.default_rng(5).choice(np.arange(1, N), 500, replace=False)] = 0
    _, on = check(rows, qs, 10, radius=radius, valid=valid)
    if radius == 650.0:  # cuts some lists short
        assert (on < 10).any() and (on == 10).any()


@pytest.mark.parametrize("k,nq,knob,kernel", [(17, NQ, None, 0), (10, 31, None, 0), (10, NQ, "0", 0), (16, 32, None, 3)])
def test_routing(monkeypatch, k, nq, knob, kernel):
    """Beyond the list length, below the batch size or with the knob off the
    quad-per-row kernel answers, with the same results."""
    if knob is not None:
        monkeypatch.setenv("NGT_AMD_LINEAR_U8", knob)
    rows, qs = random_case(128)
    check(rows, qs[:nq], k, kernel=kernel)
