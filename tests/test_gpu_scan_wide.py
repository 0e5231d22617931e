"""The matrix-core filtered exact scan for lists of 17 .. 128 results
(ngt_amd/csrc/scan_mfma_wide.hip) against the reference's scan restated on the
CPU: ids, distance bits and counts, and the kernel that ran
(DeviceIndex.last_scan_kernel() == 5).  2,881 rows: row 0 the dummy, 11 full
256-row tiles and a last tile of 65 rows, shorter than most k; 160 queries: one
full and one ragged 128-query block.  NGT_AMD_SCAN_WIDE_PARTS caps the row
parts, so that one workgroup walks several tiles (the default split of a table
this small is one tile per part: only the bootstrap tile)."""
import numpy as np
import pytest

import oracle_py as O
from ngt_amd.device import DeviceIndex, padded_dim

pytestmark = pytest.mark.gpu

N, NQ = 2881, 160
U32 = np.uint32


def oracle(metric, rows, qs, k, radius=-1.0, valid=None):
    dim, dtype = rows.shape[1], rows.dtype
    pad = np.zeros((rows.shape[0], padded_dim(dim)), dtype)
    pad[:, :dim] = rows
    qp = np.zeros((qs.shape[0], pad.shape[1]), dtype)
    qp[:, :dim] = qs
    if valid is None:
        return O.linear_search_batch(metric, pad, qp, k, radius=radius, threads=8)
    oi, od, on = np.zeros((len(qp), k), U32), np.zeros((len(qp), k), np.float32), np.zeros(len(qp), U32)
    for q in range(len(qp)):
        i, d = O.linear_search(metric, pad, qp[q], k, valid=valid, radius=radius)
        on[q], oi[q, :len(i)], od[q, :len(i)] = len(i), i, d
    return oi, od, on


def check(monkeypatch, metric, rows, qs, k, parts=None, radius=-1.0, valid=None, kernel=5, expect=None):
    if parts is None:  # the default split, whatever an earlier call of the test set
        monkeypatch.delenv("NGT_AMD_SCAN_WIDE_PARTS", raising=False)
    else:
        monkeypatch.setenv("NGT_AMD_SCAN_WIDE_PARTS", str(parts))
    ix = DeviceIndex(metric, "float" if rows.dtype == np.float32 else "uint8", rows.shape[1])
    try:
        ix.set_objects(rows, valid=valid)
        gi, gd, gn = ix.linear_search(qs.astype(np.float32), k=k, radius=radius)
        assert ix.last_scan_kernel() == kernel
    finally:
        ix.close()
    oi, od, on = expect or oracle(metric, rows, qs, k, radius, valid)
    assert np.array_equal(gn, on)
    live = np.arange(k)[None, :] < on[:, None]
    assert np.array_equal(gi[live], oi[live]), np.flatnonzero(((gi != oi) & live).any(1))[:8]
    assert np.array_equal(gd.view(U32)[live], od.view(U32)[live])
    return oi, od, on


def random_case(dim, seed=0, offset=0.0, n=N):
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, dim), np.float32)
    rows[1:] = rng.random((n - 1, dim), dtype=np.float32) + np.float32(offset)
    rows[rng.integers(1, n, 40)] = rows[rng.integers(1, n, 40)]  # exact duplicates
    qs = rng.random((NQ, dim), dtype=np.float32) + np.float32(offset)
    qs[:20] = rows[rng.integers(1, n, 20)]  # distance 0, ties by id
    return rows, qs


@pytest.mark.parametrize("dim,k", [(8, 17), (100, 33), (128, 100), (256, 128), (960, 64)])
def test_random_l2(monkeypatch, dim, k):
    rows, qs = random_case(dim)
    expect = oracle("l2", rows, qs, k)
    for parts in (None, 1, 2):  # default: a tile per part; 1: bootstrap + 11 steady tiles
        check(monkeypatch, "l2", rows, qs, k, parts, expect=expect)


@pytest.mark.parametrize("dim,k,offset", [(40, 128, -0.5), (100, 50, 0.0)])
def test_random_cosine(monkeypatch, dim, k, offset):
    rows, qs = random_case(dim, seed=1, offset=offset)
    expect = oracle("cosine", rows, qs, k)
    for parts in (1, None):
        check(monkeypatch, "cosine", rows, qs, k, parts, expect=expect)


def test_wide_margins(monkeypatch):
    """Norms far above the distances: many candidates per tile, the overflow
    and bitmap path."""
    check(monkeypatch, "l2", *random_case(128, seed=2, offset=500.0), 100, parts=1)


def test_all_rows_equal(monkeypatch):
    rng = np.random.default_rng(3)
    rows = np.repeat(rng.random((1, 32), dtype=np.float32), N, 0)
    oi, _, _ = check(monkeypatch, "l2", rows, rng.random((NQ, 32), dtype=np.float32), 128, parts=1)
    assert np.array_equal(oi, np.broadcast_to(np.arange(1, 129, dtype=U32), oi.shape))


def test_removed_rows_and_radius(monkeypatch):
    rows, qs = random_case(64, seed=4)
    rng = np.random.default_rng(5)
    valid = np.ones(N, np.uint8)
    valid[0] = 0
    valid[rng.choice(np.arange(1, N), 500, replace=False)] = 0
    valid[rng.permutation(np.arange(1, 256))[20:]] = 0  # the first tile: fewer than k live rows
    r = float(np.median(oracle("l2", rows, qs, 40, valid=valid)[1][:, 39]))
    for radius in (-1.0, 0.0, r):
        expect = oracle("l2", rows, qs, 40, radius, valid)
        for parts in (1, None):
            _, _, on = check(monkeypatch, "l2", rows, qs, 40, parts, radius=radius, valid=valid, expect=expect)
        if radius == r:
            assert (on < 40).any() and (on == 40).any()


def test_tiny_table(monkeypatch):
    """k clamps to the 99 live rows: every one comes back, in order."""
    rows, qs = random_case(128, seed=6, n=100)
    _, _, on = check(monkeypatch, "l2", rows, qs, 128)
    assert (on == 99).all()


@pytest.mark.parametrize("metric,otype,k,nq,knob,kernel", [
    ("l2", "float", 16, NQ, None, 2), ("l2", "float", 17, NQ, None, 5), ("l2", "float", 33, NQ, None, 5),
    ("l2", "float", 128, NQ, None, 5), ("l2", "float", 129, NQ, None, 0), ("l2", "float", 100, 31, None, 0),
    ("l2", "float", 100, NQ, "0", 0), ("cosine", "float", 17, NQ, None, 5), ("l2", "uint8", 17, NQ, None, 0)])
def test_routing(monkeypatch, metric, otype, k, nq, knob, kernel):
    """Lists of 17 .. 128 results of 32 or more float L2 / Cosine queries take
    the wide kernel (at k = 17 .. 32 it was measured against the query-tiled
    FMA scan it replaces); every other call keeps its kernel,
    with the same results."""
    if knob is not None:
        monkeypatch.setenv("NGT_AMD_LINEAR_WIDE", knob)
    rows, qs = random_case(128)
    if otype == "uint8":
        rows, qs = (rows * 255).astype(np.uint8), (qs * 255).astype(np.uint8)
    check(monkeypatch, metric, rows, qs[:nq], k, kernel=kernel)
