"""The scripts, the heap model and the radii of test_gpu_unchecked_set.py,
checked without a GPU: what that test expects of the device is only as good
as these."""
import numpy as np
import pytest

import test_gpu_unchecked_set as T


@pytest.mark.parametrize("order", T.ORDERS)
def test_scripts_and_model(order):
    script, d = T.script_of(order)
    keys = script[script != 0]
    assert len(keys) == T.N and len(set(keys.tolist())) == T.N  # distinct keys, none 0 or ~0
    assert keys.max() < np.uint64(0xFFFFFFFFFFFFFFFF)
    assert int((script == 0).sum()) >= T.N + 1  # drained, and one pop more
    popped, largest = T.model(script)
    # every key comes out once, then nothing; a key order is a (distance, id) order
    assert sorted(k for k in popped if k) == sorted(keys.tolist()) and popped[-1] == 0
    by_dist_id = sorted(zip(d.tolist(), range(1, T.N + 1)))
    assert sorted(keys.tolist()) == [int(T.make_keys([a], [b])[0]) for a, b in by_dist_id]
    assert [T.key_dist(k) for k in sorted(keys.tolist())[:3]] == [a for a, _ in by_dist_id[:3]]
    if order == "interleaved":
        assert largest == T.N - T.N // 8 + 1 and popped[:T.N // 8] != sorted(keys.tolist())[:T.N // 8]
    else:
        assert largest == T.N and popped[:T.N] == sorted(keys.tolist())
    if order == "lattice":
        assert len(set(d.tolist())) == 4 and int((d == d.min()).sum()) == 750


@pytest.mark.parametrize("order", T.ORDERS)
def test_radii(order):
    script, d = T.script_of(order)
    popped, _ = T.model(script)
    expr = float(np.median(d))
    within = int((d <= np.float32(expr)).sum())
    assert T.N // 4 <= within < T.N  # some keys beyond the radius, many within
    if order != "interleaved":
        assert len(T.cut(popped, expr)) == within
    tr = T.trim_radius(d)
    assert int((d <= np.float32(tr)).sum()) < 256
    assert T.cut(popped, T.FLT_MAX) == [k for k in popped if k][:len(T.cut(popped, T.FLT_MAX))]
