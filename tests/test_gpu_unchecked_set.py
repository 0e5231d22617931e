"""The unchecked set of the latency and NGTQG search kernels
(ngt_amd/csrc/unchecked_set.h) against a plain heap.

ngt_amd_test_unchecked_set runs a script of inserts and pops on one wave with
the instantiation a kernel uses -- LAT = UncheckedSet<tagged, no trim>
(search_lat.hip), QG = UncheckedSet<untagged, trim> (qg_kernels.hip) -- and
returns what it popped, its largest size and its error word.  The expected
side of every assertion is the pure-Python model below (heapq); the scripts
and the choices of the exploration radius are checked without a GPU in
test_unchecked_set_model.py.

Shapes: 3000 keys; tail capacities 64 and 128 (the smallest the
NGT_AMD_LAT_TAIL and NGT_AMD_CQ_CAP knobs allow), so the head, the tail and the
spill all fill and refill many times; spill capacity 4096 (enough) or 256
(too small for the keys within the radius, or enough only after trimming)."""
import heapq

import numpy as np
import pytest

import ngt_amd

pytestmark = pytest.mark.gpu

N = 3000
FLT_MAX = float(np.finfo(np.float32).max)
ORDERS = ["ascending", "descending", "random", "lattice", "interleaved"]
LAT = (1, 0)  # (tagged, trim) of search_lat.hip
QG = (0, 1)   # of qg_kernels.hip
NO_LANE = 0xFF


def make_keys(dists, ids):
    """(distance, id) keys as the kernels order them (ngt_device.h make_key;
    distances here are positive)."""
    o = np.asarray(dists, np.float32).view(np.uint32) | np.uint32(0x80000000)
    return (o.astype(np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)


def key_dist(key):
    return float(np.array([(int(key) >> 32) & 0x7FFFFFFF], np.uint32).view(np.float32)[0])


def keys_of(order):
    """The N keys of a case in insertion order, and their distances."""
    rng = np.random.default_rng(20240611)
    ids = np.arange(1, N + 1)
    if order == "lattice":
        # 4 distinct distances x 750 ids: more keys than any threshold asks
        # for share the smallest distance
        d = np.repeat(np.array([0.5, 1.0, 1.5, 2.0], np.float32), N // 4)
    else:
        d = (1.0 + np.arange(N) * 0.001).astype(np.float32)
    keys = make_keys(d, ids)
    if order == "ascending":
        pass
    elif order == "descending":
        keys = keys[::-1]
    else:
        keys = keys[rng.permutation(N)]
    return keys.copy(), d


def script_of(order):
    """Insert everything, then drain (one pop more than there are keys);
    'interleaved' pops once per 8 inserts first, as a search does."""
    keys, d = keys_of(order)
    if order == "interleaved":
        words = []
        for i, k in enumerate(keys):
            words.append(int(k))
            if i % 8 == 7:
                words.append(0)
    else:
        words = [int(k) for k in keys]
    words += [0] * (N + 1)
    return np.array(words, np.uint64), d


def model(script):
    """heapq: the popped keys (0 from an empty heap) and the largest size."""
    heap, popped, largest = [], [], 0
    for w in script.tolist():
        if w:
            heapq.heappush(heap, w)
            largest = max(largest, len(heap))
        else:
            popped.append(heapq.heappop(heap) if heap else 0)
    return popped, largest


def cut(popped, expr):
    """Up to the first pop that gave nothing or a key beyond the radius: keys
    beyond it may be dropped at any refill, and a search stops there."""
    out = []
    for k in popped:
        if k == 0 or key_dist(k) > expr:
            break
        out.append(k)
    return out


def run(inst, script, tail_cap, spill_cap, expr, tag_lane=None):
    L = ngt_amd.lib()
    tagged, trim = inst
    n = len(script)
    script = np.ascontiguousarray(script, np.uint64)
    lanes = np.full(n, NO_LANE, np.uint8) if tag_lane is None else np.ascontiguousarray(tag_lane, np.uint8)
    popped = np.zeros(n, np.uint64)
    events = np.zeros((3 * n, 2), np.uint64)
    cnt = np.zeros(4, np.uint32)  # npopped, nevents, maxq, error
    p = cnt.ctypes.data
    rc = L.ngt_amd_test_unchecked_set(0, tagged, trim, script.ctypes.data, lanes.ctypes.data, n, tail_cap, spill_cap,
                                      expr, popped.ctypes.data, p, events.ctypes.data, p + 4, p + 8, p + 12)
    assert rc == 0, L.ngt_amd_last_error()
    assert int(cnt[0]) == int((script == 0).sum())
    return popped[:cnt[0]].tolist(), int(cnt[2]), int(cnt[3]), events[:cnt[1]].tolist()


@pytest.mark.parametrize("inst", [LAT, QG], ids=["lat", "qg"])
@pytest.mark.parametrize("tail_cap", [64, 128])
@pytest.mark.parametrize("order", ORDERS)
def test_pops_in_key_order(order, tail_cap, inst):
    script, _ = script_of(order)
    want, largest = model(script)
    got, maxq, err, _ = run(inst, script, tail_cap, 4096, FLT_MAX)
    print("maxq %d (model %d) error %d" % (maxq, largest, err))
    assert got == want
    assert err == 0
    assert maxq == largest


@pytest.mark.parametrize("inst", [LAT, QG], ids=["lat", "qg"])
@pytest.mark.parametrize("tail_cap", [64, 128])
@pytest.mark.parametrize("order", ORDERS)
def test_finite_radius(order, tail_cap, inst):
    script, d = script_of(order)
    expr = float(np.median(d))
    want, _ = model(script)
    got, _, err, _ = run(inst, script, tail_cap, 4096, expr)
    assert cut(got, expr) == cut(want, expr)
    assert len(cut(want, expr)) >= N // 4
    assert err == 0


@pytest.mark.parametrize("tail_cap", [64, 128])
@pytest.mark.parametrize("order", ORDERS)
def test_full_spill_is_reported(order, tail_cap):
    """Without trimming, more keys within the radius than the three levels
    hold: the capacity bit and nothing else."""
    script, _ = script_of(order)
    _, _, err, _ = run(LAT, script, tail_cap, 256, FLT_MAX)
    assert err == 1


@pytest.mark.parametrize("tail_cap", [64, 128])
@pytest.mark.parametrize("order", ORDERS)
def test_trim_makes_room(order, tail_cap):
    """With trimming and fewer than 256 keys within the radius, the spill
    never stays full."""
    script, d = script_of(order)
    expr = trim_radius(d)
    assert int((d <= np.float32(expr)).sum()) < 256
    want, _ = model(script)
    got, _, err, _ = run(QG, script, tail_cap, 256, expr)
    assert err == 0
    assert cut(got, expr) == cut(want, expr)


def trim_radius(d):
    """A radius with fewer than 256 keys within it: the 200th smallest
    distance, or, where more keys than that share the smallest one (the
    lattice), half of it -- no key within."""
    s = np.sort(d)
    return float(s[199]) if s[199] < s[255] else float(s[0]) / 2


def tag_script(order):
    """Tags for the head: lane 0 after every insert of the interleaved script
    (the next pop takes it back), lanes spread over the head otherwise (the
    descending inserts push each of them out of the full head's end)."""
    script, _ = script_of(order)
    n = len(script)
    lanes = np.full(n, NO_LANE, np.uint8)
    ins = script != 0
    if order == "interleaved":
        lanes[ins] = 0
    else:
        lanes[ins] = (np.arange(n)[ins] * 7 % 64).astype(np.uint8)
    return script, lanes


@pytest.mark.parametrize("tail_cap", [64, 128])
@pytest.mark.parametrize("order", ["descending", "random", "interleaved"])
def test_tags_come_back_once(order, tail_cap):
    script, lanes = tag_script(order)
    want, _ = model(script)
    got, _, err, events = run(LAT, script, tail_cap, 4096, FLT_MAX, lanes)
    assert got == want and err == 0
    out, given, back, orphaned = {}, 0, 0, 0
    for head, key in events:
        kind, tag = head >> 32, head & 0xFFFFFFFF
        assert tag < 64
        if kind == 1:  # tagged: nobody holds this tag
            assert tag not in out
            out[tag] = key
            given += 1
        elif kind == 2:  # popped with its tag: the key that was tagged
            assert out.pop(tag, None) == key
            back += 1
        else:  # orphaned: the tag of a key that left the head for the tail
            assert kind == 3 and tag in out
            del out[tag]
            orphaned += 1
    print("tags given %d, popped %d, orphaned %d" % (given, back, orphaned))
    assert not out  # the set was drained: every tag came back
    assert given == back + orphaned and given > 0
    if order == "descending":
        assert orphaned > 0
    if order == "interleaved":
        assert back > 0
