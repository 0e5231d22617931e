"""Adversarial inputs for the two filters that rest on a hand-derived bound
instead of restating the reference's arithmetic:

* the 1-byte filter copy of the graph search (filter_kernels.hip; filter_l2u8,
  filter_threshold, cos_filter_bound in search_common.h; consumed by
  search_kernels.hip, search_la.hip and search_lat.hip), and
* the matrix-core exact scan (scan_mfma.hip with scan_kappa, rho and the
  2^-100 slack of ngt_amd_api.cpp).

Bar: a filtered search returns the ids, the float distance bits, the result
counts and the reference's counters of the unfiltered search and of the oracle
restatement -- on data chosen against the derivations: one outlier element
(b huge, every other code 0), a range wider than FLT_MAX (b = inf), a narrow
cluster far from the origin (b of a few ulps), lattices with few levels (ties
exactly on the radius), queries far outside the rows' range (the clamp step),
data at 2^-40 and 2^+40 (the absolute slack terms), mixed signs (a < 0),
constant rows (b = 0) and, for cosine, rows whose norm is of the order of E.
The classes that must reject prove the filter is not idle.

Non-vacuity.  On uniform, cluster, mixed_sign and both scales the filtered
run must make strictly fewer exact evaluations (counter column 6, summed over
the queries) than the unfiltered one, per search setting, with the full
visited set.  Three places where that cannot hold, each for a reason in the
maths and not in the device:

* The latency kernel (search_lat.hip) reports in column 6 the fresh neighbours
  of the committed expansions (its speculation waves evaluate ahead of the
  commits, and how far depends on timing), so the column equals the
  unfiltered run's by construction; that form asserts equality of results and
  counters only.
* L2 `cluster` at D = 90 and 120: the pad zeros join the range, so a = 0 and
  b = 1000.001 / 255 = 3.92; every real element (1000 .. 1000.001) gets code
  255 and every query byte is 255, the integer sum S is 0 for every row and
  never exceeds a threshold.  The bound is useless there, not wrong (the
  results are still compared).  At D = 96 and 128 the class rejects.
* Cosine / angle `cluster`: all cosines lie within 1e-12 of 1, far inside the
  2e-5 slack of cos_filter_bound, so no bound can separate two rows.  This
  class is the one that showed the cosine bound unsound: the comparator's
  1 - cs comes out at -6e-8 .. -1.2e-7 for such rows, the exploration radius
  turns negative, and a bound floored at 0 threw true neighbours away.

Every case prints its exact-evaluation totals (counter column 6) as
"adv-col6 ..." lines before it asserts.
"""
import functools
import os

import numpy as np
import pytest

import oracle_py as O
from ngt_amd.device import SEED_GIVEN, DeviceIndex
from test_gpu_parity import _random_graph

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
U32 = np.uint32

L2_CLASSES = ["uniform", "outlier_linked", "outlier_isolated", "cluster", "binary", "ternary", "far_queries",
              "scale_small", "scale_large", "mixed_sign", "constant"]
# classes whose filtered run must evaluate strictly fewer exact distances
L2_MUST_REJECT = {"uniform", "cluster", "mixed_sign", "scale_small", "scale_large"}
COS_CLASSES = ["uniform", "mixed_sign", "tiny_norm", "outlier_linked", "cluster", "scale_small", "scale_large"]
COS_MUST_REJECT = {"uniform"}  # not cluster: module docstring


# ---------------------------------------------------------------------------
# one generator for rows and queries (pure numpy, fixed seeds, row 0 the dummy)
# ---------------------------------------------------------------------------
def _seed(cls, n, dim):
    return [sum(ord(c) for c in cls), n, dim]


@functools.lru_cache(maxsize=None)
def _graph(n, deg):
    _, offs, edges = _random_graph(n, 1, deg, 1000 + deg)
    return offs, edges


@functools.lru_cache(maxsize=None)
def make(cls, n, dim, nq, big=2.5e38):
    """rows [n (+2 for outlier_isolated), dim] and queries [nq, dim] of the
    class; `big` is the magnitude of the two isolated outlier elements."""
    rng = np.random.default_rng(_seed(cls, n, dim))
    u = lambda *s: rng.random(s, dtype=np.float32)  # noqa: E731
    rows = np.zeros((n, dim), np.float32)
    if cls in ("uniform", "far_queries", "outlier_linked", "outlier_isolated", "constant"):
        rows[1:] = u(n - 1, dim)
        qs = u(nq, dim)
        if cls == "far_queries":
            qs[:nq // 2] = np.float32(5) + np.float32(3) * qs[:nq // 2]
            qs[nq // 2:] = np.float32(-4) * qs[nq // 2:]
        elif cls == "outlier_linked":
            rows[n // 3, dim // 2] = np.float32(1e6)
        elif cls == "outlier_isolated":
            ext = u(2, dim)
            ext[0, 3] = np.float32(big)
            ext[1, dim - 2] = np.float32(-big)
            rows = np.concatenate([rows, ext])
        elif cls == "constant":
            rows[1:] = np.float32(0.25)
    elif cls == "cluster":
        rows[1:] = np.float32(1000) + np.float32(1e-3) * u(n - 1, dim)
        qs = np.float32(1000) + np.float32(1e-3) * u(nq, dim)
    elif cls in ("binary", "ternary"):
        lv = 2 if cls == "binary" else 3
        rows[1:] = rng.integers(0, lv, (n - 1, dim)).astype(np.float32)
        qs = rows[rng.integers(1, n, nq)].copy()
        for i in range(nq):  # one or two elements moved to the next level
            j = rng.choice(dim, 1 + i % 2, replace=False)
            qs[i, j] = (qs[i, j] + 1) % lv
    elif cls in ("scale_small", "scale_large"):
        e = -40 if cls == "scale_small" else 40
        rows[1:] = np.ldexp(u(n - 1, dim), e)
        qs = np.ldexp(u(nq, dim), e)
    elif cls in ("mixed_sign", "tiny_norm"):
        rows[1:] = np.float32(2) * u(n - 1, dim) - np.float32(1)
        qs = np.float32(2) * u(nq, dim) - np.float32(1)
        if cls == "tiny_norm":
            rows[7::7] *= np.float32(1e-6)
    else:
        raise KeyError(cls)
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs


def _pad(x, dim):
    dp = ((dim - 1) // 16 + 1) * 16
    if x.shape[1] == dp:
        return x
    p = np.zeros((x.shape[0], dp), np.float32)
    p[:, :x.shape[1]] = x
    return p


@functools.lru_cache(maxsize=None)
def _case(metric, cls, n, dim, deg, nq):
    """Rows, queries, graph (with edge-less, in-edge-less extra rows for
    outlier_isolated), seeds and the class's median query-to-row distance."""
    rows, qs = make(cls, n, dim, nq)
    offs, edges = _graph(n, deg)
    if rows.shape[0] > n:
        offs = np.concatenate([offs, np.repeat(offs[-1:], rows.shape[0] - n)])
    if cls == "outlier_linked":
        assert (edges == n // 3).any()  # the outlier row is reachable
    rng = np.random.default_rng(_seed(cls, nq, deg))
    seeds = np.stack([rng.choice(np.arange(1, n), 10, replace=False) for _ in range(nq)]).astype(np.uint32)
    # median distance in double over the first queries and the ordinary rows
    r, q = rows[1:n].astype(np.float64), qs[:24].astype(np.float64)
    dot = q @ r.T
    if metric == "l2":
        d = np.sqrt(np.maximum((q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2 * dot, 0.0))
    else:
        cs = dot / np.sqrt((q * q).sum(1)[:, None] * (r * r).sum(1)[None, :])
        d = 1.0 - cs if metric == "cosine" else np.arccos(np.clip(cs, -1.0, 1.0))
    radius = float(np.float32(np.median(d)))
    return rows, qs, offs, edges, seeds, radius


def _settings(radius):
    return [(0.0, None), (0.1, None), (-0.05, None), (0.2, radius)]


@functools.lru_cache(maxsize=None)
def _oracle(metric, cls, n, dim, deg, nq, nuse, k, si):
    rows, qs, offs, edges, seeds, radius = _case(metric, cls, n, dim, deg, nq)
    eps, rad = _settings(radius)[si]
    kw = {} if rad is None else {"radius": rad}
    return O.search_batch(metric, _pad(rows, dim), offs, edges, _pad(qs[:nuse], dim), seeds[:nuse], k,
                          np.float32(eps), edge_size=0, threads=THREADS, **kw)


@pytest.fixture(scope="module")
def pool():
    """Device indexes shared by the cases of one (metric, class, shape)."""
    made = {}

    def get(metric, cls, n, dim, deg, nq):
        key = (metric, cls, n, dim, deg)
        if key not in made:
            rows, _, offs, edges, _, _ = _case(metric, cls, n, dim, deg, nq)
            ix = DeviceIndex(metric, "float", dim)
            ix.set_objects(rows)
            ix.set_graph(offs, edges)
            made[key] = ix
        return made[key]

    yield get
    for ix in made.values():
        ix.close()


def _live(n, k):
    return np.arange(k)[None, :] < n[:, None]


def _check_search(monkeypatch, pool, metric, cls, n, dim, deg, k, la, nq, nuse, visited_modes, want_form,
                  must_reject):
    """Filtered against unfiltered against the oracle, for the four search
    settings and the given visited-set modes of one kernel form."""
    monkeypatch.setenv("NGT_AMD_LA", la)
    rows, qs, offs, edges, seeds, radius = _case(metric, cls, n, dim, deg, nq)
    ix = pool(metric, cls, n, dim, deg, nq)
    q, sd = qs[:nuse], list(seeds[:nuse])
    for vis in visited_modes:
        for si, (eps, rad) in enumerate(_settings(radius)):
            tag = (metric, cls, dim, la, vis, eps, rad)
            kw = dict(k=k, epsilon=eps, radius=-1.0 if rad is None else rad, edge_size=0, seed_mode=SEED_GIVEN,
                      seeds=sd, visited_hash_log2=vis)
            fi, fd, fn, fc = ix.search(q, distance_filter=1, **kw)
            assert ix.last_search_filtered(), tag
            assert ix.last_search_lookahead() == want_form, tag
            ui, ud, un, uc = ix.search(q, distance_filter=-1, **kw)
            assert not ix.last_search_filtered(), tag
            oi, od, on, oc = _oracle(metric, cls, n, dim, deg, nq, nuse, k, si)
            fc, uc = fc.astype(np.int64), uc.astype(np.int64)
            print("adv-col6", metric, cls, dim, "la=" + la, "vis=%d" % vis, "eps=%g" % eps,
                  "radius=%s" % rad, "filtered", int(fc[:, 6].sum()), "unfiltered", int(uc[:, 6].sum()))
            # the bound: filtered == unfiltered
            assert np.array_equal(fn, un), tag
            m = _live(un, k)
            assert np.array_equal(fi[m], ui[m]), tag
            assert np.array_equal(fd.view(U32)[m], ud.view(U32)[m]), tag
            # [5] depends on the kernel's compaction points; with the
            # accepted-only set [0]/[1] count evaluations, which depend on the
            # kernel (test_distance_filter_identical): the traversal counters
            for col in ((0, 1, 2, 4, 7) if vis != -2 else (2, 4, 7)):
                assert np.array_equal(fc[:, col], uc[:, col]), tag + (col,)
            # the search: device == oracle
            assert np.array_equal(fn, on), tag
            m = _live(on, k)
            assert np.array_equal(fi[m], oi[m]), tag
            assert np.array_equal(fd.view(U32)[m], od.view(U32)[m]), tag
            if vis != -2:
                assert np.array_equal(fc[:, 0], oc[:, 0].astype(np.int64)), tag
                assert np.array_equal(fc[:, 2], oc[:, 2].astype(np.int64)), tag
                if must_reject:
                    assert fc[:, 6].sum() < uc[:, 6].sum(), tag
            else:
                assert (fc[:, 0] >= oc[:, 0].astype(np.int64)).all(), tag


# kernel form -> (NGT_AMD_LA, queries, visited-set modes, last_search_lookahead)
FORMS = {
    "one": ("0", 24, (0, -1, -2), -1),  # one expansion per pop; -2: the chunked accepted-only path
    "wave": ("1", 600, (0, -2), 0),     # lookahead, a wave per query
    "lat": ("2", 24, (0,), 1),          # latency launches
}


# ---------------------------------------------------------------------------
# graph search, L2 filter
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cls", L2_CLASSES)
def test_l2_filter_adversarial(monkeypatch, pool, cls, form):
    """D = 128 (NCH = 8): every class on every kernel form."""
    la, nuse, vms, want = FORMS[form]
    _check_search(monkeypatch, pool, "l2", cls, 4000, 128, 24, 20, la, 600, nuse, vms, want,
                  cls in L2_MUST_REJECT and form != "lat")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dim", [96, 90, 120])
@pytest.mark.parametrize("cls", ["uniform", "cluster", "ternary"])
def test_l2_filter_adversarial_padded_widths(monkeypatch, pool, cls, dim, form):
    """Dp = 96 (NCH = 6, the odd-NW branch of load_code_words) and dims whose
    pad zeros take part in the (a, b) range: 90 -> 96, 120 -> 128."""
    la, nuse, vms, want = FORMS[form]
    useless = cls == "cluster" and dim % 16 != 0  # a = 0: every code 255 (module docstring)
    _check_search(monkeypatch, pool, "l2", cls, 4000, dim, 24, 20, la, 600, nuse, vms, want,
                  cls in L2_MUST_REJECT and form != "lat" and not useless)


# ---------------------------------------------------------------------------
# graph search, cosine / angle filter
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [192, 256, 250])
@pytest.mark.parametrize("metric", ["cosine", "angle"])
@pytest.mark.parametrize("cls", COS_CLASSES)
def test_cosine_filter_adversarial(monkeypatch, pool, cls, metric, dim):
    _check_search(monkeypatch, pool, metric, cls, 2500, dim, 16, 10, "0", 24, 24, (-1, 0), -1,
                  cls in COS_MUST_REJECT)


# ---------------------------------------------------------------------------
# batch scan (matrix-core filter)
# ---------------------------------------------------------------------------
def _check_scan(metric, rows, qs, dim, valid=None):
    ix = DeviceIndex(metric, "float", dim)
    ix.set_objects(rows, valid=valid)
    pad, qp = _pad(rows, dim), _pad(qs, dim)
    nq = qs.shape[0]
    try:
        for k in (10, 16):
            gi, gd, gn = ix.linear_search(qs, k=k)
            if valid is None:
                oi, od, on = O.linear_search_batch(metric, pad, qp, k, threads=THREADS)
            else:
                oi, od, on = np.zeros((nq, k), U32), np.zeros((nq, k), np.float32), np.zeros(nq, U32)
                for q in range(nq):
                    i, d = O.linear_search(metric, pad, qp[q], k, valid=valid)
                    on[q] = len(i)
                    oi[q, :len(i)], od[q, :len(i)] = i, d
            assert np.array_equal(gn, on), k
            m = _live(on, k)
            assert np.array_equal(gi[m], oi[m]), (k, np.flatnonzero((gi != oi).any(1))[:8])
            assert np.array_equal(gd.view(U32)[m], od.view(U32)[m]), k
            # equal distances come out ranked by id
            tie = (gd[:, 1:] == gd[:, :-1]) & m[:, 1:]
            assert (gi[:, 1:][tie] > gi[:, :-1][tie]).all(), k
    finally:
        ix.close()


SCAN_N, SCAN_NQ = 3001, 160  # one full and one ragged 128-query block


@pytest.mark.parametrize("dim", [24, 100, 128])
@pytest.mark.parametrize("cls", L2_CLASSES + ["outlier_isolated_valid"])
def test_scan_l2_adversarial(cls, dim):
    """k = 10 and 16 against the oracle.  outlier_isolated: the two rows of
    +-2.5e38 stay in the table but are marked removed; the _valid variant
    keeps them valid with +-1e18, so Xmax dwarfs every other norm."""
    valid = None
    if cls == "outlier_isolated_valid":
        rows, qs = make("outlier_isolated", SCAN_N, dim, SCAN_NQ, 1e18)
    else:
        rows, qs = make(cls, SCAN_N, dim, SCAN_NQ)
        if cls == "outlier_isolated":
            valid = np.ones(rows.shape[0], np.uint8)
            valid[0] = 0
            valid[SCAN_N:] = 0
    _check_scan("l2", rows, qs, dim, valid)


@pytest.mark.parametrize("dim", [40, 100])
@pytest.mark.parametrize("cls", ["mixed_sign", "tiny_norm", "outlier_linked", "cluster", "scale_small",
                                 "scale_large"])
def test_scan_cosine_adversarial(cls, dim):
    rows, qs = make(cls, SCAN_N, dim, SCAN_NQ)
    _check_scan("cosine", rows, qs, dim)
