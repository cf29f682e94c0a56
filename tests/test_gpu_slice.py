"""GPU: the window slices (gsamd.Slice, the gs_slice_* calls) against a restatement of the
contract in numpy: build the entries of the direction, group them by key with a stable sort
(arrival order inside a vertex, vertices ascending in signed order) and reduce each group with
int64 arithmetic, so sums wrap. Everything is an integer: every comparison is exact. The
reference's pinned outputs (tests/golden/slice_pins.json, TestSlice.java) are section 1. The
shape cases sit at the tile of the reduce kernel (T = gsamd.SLICE_TILE) and at the positions a
thread (T / 256) and a wave (64) own; stats() proves that a case really crossed tiles."""
import ctypes
import json
import os

import numpy as np
import pytest

import gsamd

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
SENTINEL = -0x5A5A5A5A5A5A5A5B
T = gsamd.SLICE_TILE
PER = T // 256
DIRECTIONS = ("out", "in", "all")
OPS = ("sum", "min", "max", "count")


def _entries(src, dst, val, direction):
    """(key, neighbour, value) of every entry, in arrival order."""
    s, d = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    w = None if val is None else np.asarray(val, np.int64)
    if direction == "out":
        return s, d, w
    if direction == "in":
        return d, s, w
    key = np.stack([s, d], axis=1).ravel()  # the edge, then its reverse
    nb = np.stack([d, s], axis=1).ravel()
    return key, nb, None if w is None else np.repeat(w, 2)


def _truth(src, dst, val, direction):
    """vertex, offset, neighbor, val of the CSR and {op: one value per vertex}."""
    key, nb, w = _entries(src, dst, val, direction)
    order = np.argsort(key, kind="stable")
    k = key[order]
    heads = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]])) if len(k) else np.zeros(0, np.int64)
    offset = np.concatenate([heads, [len(k)]]).astype(np.uint64)
    red = {"count": np.diff(offset.astype(np.int64))}
    if w is not None:
        wv = w[order]
        with np.errstate(over="ignore"):
            for op, fn in (("sum", np.add), ("min", np.minimum), ("max", np.maximum)):
                red[op] = fn.reduceat(wv, heads) if len(k) else np.zeros(0, np.int64)
    return k[heads] if len(k) else k, offset, nb[order], None if w is None else w[order], red


def _check(sl, src, dst, val, direction, ops=OPS):
    """Fold the window and compare every read with the truth; returns the truth."""
    v, off, nb, wv, red = _truth(src, dst, val, direction)
    sl.window(src, dst, val, direction)
    assert sl.size() == (len(v), len(nb))
    for op in ops:
        if op != "count" and val is None:
            continue
        gv, gr = sl.reduce(op)
        assert gv.dtype == np.int64 and gr.dtype == np.int64
        assert np.array_equal(gv, v), (direction, op)
        assert np.array_equal(gr, red[op]), (direction, op)
    gv, goff, gnb, gw = sl.neighborhoods()
    assert np.array_equal(gv, v) and np.array_equal(goff, off), direction
    assert np.array_equal(gnb, nb), direction
    assert (gw is None) if wv is None else np.array_equal(gw, wv), direction
    return v, off, nb, wv, red


def _pins():
    with open(os.path.join(GOLD, "slice_pins.json")) as f:
        return json.load(f)


# ---- 1. the reference's pinned outputs
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_pins(gs, direction):
    pins = _pins()
    e = np.array(pins["edges"]["rows"], np.int64)
    with gs.Slice() as sl:
        sl.window(e[:, 0], e[:, 1], e[:, 2], direction)
        v, s = sl.reduce("sum")
        assert [list(r) for r in zip(v.tolist(), s.tolist())] == pins["sum_" + direction]["rows"]
        v, off, nb, w = sl.neighborhoods()
        rows = []
        for k in range(len(v)):  # applyOnNeighbors: sum the edge values of the neighbourhood
            total = int(w[int(off[k]):int(off[k + 1])].sum())
            rows.append([int(v[k]), "big" if total > pins["threshold"]["value"] else "small"])
        assert rows == pins["apply_" + direction]["rows"]
        _check(sl, e[:, 0], e[:, 1], e[:, 2], direction)


# ---- 2. the smallest windows
def test_empty_one_and_self_loop(gs):
    with gs.Slice() as sl:
        z = np.zeros(0, np.int64)
        for direction in DIRECTIONS:
            _check(sl, z, z, z, direction)
            assert sl.size() == (0, 0)
            _check(sl, [5], [9], [-3], direction)
        v, off, nb, w, red = _check(sl, [7], [7], [11], "out")
        assert v.tolist() == [7] and nb.tolist() == [7]
        _check(sl, [7], [7], [11], "in")
        v, off, nb, w, red = _check(sl, [7], [7], [11], "all")  # a loop and its reverse: two entries
        assert v.tolist() == [7] and off.tolist() == [0, 2] and nb.tolist() == [7, 7] and w.tolist() == [11, 11]
        assert red["sum"].tolist() == [22] and red["count"].tolist() == [2]


# ---- 3. tile sizes: every key distinct, every key equal
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_tile_sizes(gs, n):
    rng = np.random.default_rng(n)
    val = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    distinct = rng.permutation(n).astype(np.int64) - n // 2
    with gs.Slice() as sl:
        _check(sl, distinct, distinct[::-1].copy(), val, "out")
        assert sl.stats()["longest"] == 1
        _check(sl, np.full(n, -4, np.int64), distinct, val, "out")
        st = sl.stats()
        assert st["longest"] == n and st["tiles"] == -(-n // T) and st["headless_tiles"] == st["tiles"] - 1
        _check(sl, distinct, np.full(n, 9, np.int64), val, "in")


# ---- 4. segments against tile, wave and thread boundaries
def _runs(lengths):
    """keys: vertex j repeated lengths[j] times, in order"""
    return np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)


def test_segment_across_tiles(gs):
    rng = np.random.default_rng(4)
    key = _runs([2, 3 * T + 1, 3])
    val = rng.integers(I64_MIN, I64_MAX, len(key), dtype=np.int64, endpoint=True)
    nb = rng.integers(-5, 5, len(key))
    with gs.Slice() as sl:
        _check(sl, key, nb, val, "out")
        st = sl.stats()
        assert st["tiles"] == 4 and st["longest"] == 3 * T + 1
        assert st["headless_tiles"] == 2  # positions T .. 3 T - 1 belong to the long vertex


def test_head_on_a_tile_boundary(gs):
    rng = np.random.default_rng(5)
    for lengths in ([T, T], [T, T, 1], [3, T - 3, T], [2 * T, T]):
        key = _runs(lengths)
        val = rng.integers(I64_MIN, I64_MAX, len(key), dtype=np.int64, endpoint=True)
        with gs.Slice() as sl:
            _check(sl, key, key + 1, val, "out")
            assert sl.stats()["longest"] == max(lengths)


@pytest.mark.parametrize("length", [63, 64, 65, PER - 1, PER, PER + 1])
def test_segment_lengths_repeated_across_a_tile(gs, length):
    rng = np.random.default_rng(length)
    key = _runs([length] * (T // length + 3))  # past one tile
    perm = rng.permutation(len(key))  # arrival order is not key order
    val = rng.integers(I64_MIN, I64_MAX, len(key), dtype=np.int64, endpoint=True)
    with gs.Slice() as sl:
        _check(sl, key[perm], perm.astype(np.int64), val, "out")
        assert sl.stats()["longest"] == length


# ---- 5. a random multigraph over hard ids, every op x every direction
def _multigraph():
    rng = np.random.default_rng(0x51CE)
    ids = np.concatenate([[I64_MIN, I64_MAX, -1, 0],
                          rng.integers(I64_MIN, I64_MAX, 296, dtype=np.int64, endpoint=True)]).astype(np.int64)
    s = ids[rng.integers(0, 300, 5000)]
    d = ids[rng.integers(0, 300, 5000)]
    w = rng.integers(I64_MIN, I64_MAX, 5000, dtype=np.int64, endpoint=True)
    w[:4] = [I64_MIN, I64_MAX, I64_MIN, I64_MAX]
    return s, d, w


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_random_multigraph(gs, direction):
    s, d, w = _multigraph()
    with gs.Slice() as sl:
        v, off, nb, wv, red = _check(sl, s, d, w, direction)
        assert {I64_MIN, I64_MAX, -1, 0} <= set(v.tolist())
        # the sums really wrapped somewhere: the exact sums differ from the int64 ones
        exact = [sum(int(x) for x in wv[int(off[k]):int(off[k + 1])]) for k in range(len(v))]
        assert any(e != int(r) for e, r in zip(exact, red["sum"]))


# ---- 6. arrival order
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_arrival_order(gs, direction):
    rng = np.random.default_rng(6)
    n = 3 * T
    s = rng.integers(0, 40, n).astype(np.int64)
    d = rng.integers(0, 40, n).astype(np.int64)
    far = np.array([0, T + 5, 2 * T + 9, 3 * T - 1])  # one vertex's entries more than T apart
    s[s == 77] = 0
    s[far] = 77
    d[far] = [3, 3, 3, 3]  # and the same (src, dst) pair again and again
    s[10:20] = 8
    d[10:20] = 9  # repeated pairs next to each other
    w = np.arange(n, dtype=np.int64) * 1000 + 1  # every value names its edge
    with gs.Slice() as sl:
        v, off, nb, wv, red = _check(sl, s, d, w, direction)
        if direction != "in":
            k = int(np.searchsorted(v, 77))
            mine = wv[int(off[k]):int(off[k + 1])]
            assert [x for x in mine.tolist() if (x - 1) // 1000 in far.tolist()] == (far * 1000 + 1).tolist()


# ---- 7. streams without values
def test_null_values(gs):
    s, d, _ = _multigraph()
    with gs.Slice() as sl:
        for direction in DIRECTIONS:
            v, off, nb, wv, red = _check(sl, s, d, None, direction)
            assert wv is None and red["count"].sum() == len(nb)
            with pytest.raises(gs.GSError) as e:
                sl.reduce("sum")
            assert e.value.code == gs.GS_ERR_INVALID
        # a val output on a window without values is invalid too
        nv, ne = sl.size()
        hv, ho, hn, hw = np.zeros(nv, np.int64), np.zeros(nv + 1, np.uint64), np.zeros(ne, np.int64), np.zeros(ne, np.int64)
        a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert gs.lib().gs_slice_neighborhoods(sl.handle, hv.ctypes.data, ho.ctypes.data, hn.ctypes.data, hw.ctypes.data,
                                               nv, ne, ctypes.byref(a), ctypes.byref(b)) == gs.GS_ERR_INVALID
        # unknown direction and op
        assert gs.lib().gs_slice_window(sl.handle, s.ctypes.data, d.ctypes.data, None, 5, 3) == gs.GS_ERR_INVALID
        assert gs.lib().gs_slice_reduce(sl.handle, 4, hv.ctypes.data, hv.ctypes.data, nv, ctypes.byref(a)) == gs.GS_ERR_INVALID


# ---- 8. truncation: the counts set, nothing written
def test_truncation(gs):
    import torch
    s, d, w = _multigraph()
    lib = gs.lib()
    with gs.Slice() as sl:
        sl.window(s, d, w, "all")
        nv, ne = sl.size()
        dev = torch.device("cuda", sl.device)
        got = ctypes.c_size_t(99)
        hv, ho = np.full(nv, SENTINEL, np.int64), np.full(nv, SENTINEL, np.int64)
        assert lib.gs_slice_reduce(sl.handle, 0, hv.ctypes.data, ho.ctypes.data, nv - 1, ctypes.byref(got)) == gs.GS_ERR_TRUNCATED
        assert got.value == nv and (hv == SENTINEL).all() and (ho == SENTINEL).all()
        tv = torch.full((nv,), SENTINEL, dtype=torch.int64, device=dev)
        to = torch.full((nv,), SENTINEL, dtype=torch.int64, device=dev)
        sl.wait_stream("torch")
        got.value = 99
        assert lib.gs_slice_reduce_device(sl.handle, 0, tv.data_ptr(), to.data_ptr(), nv - 1, ctypes.byref(got)) == gs.GS_ERR_TRUNCATED
        sl.sync()
        assert got.value == nv and bool((tv == SENTINEL).all()) and bool((to == SENTINEL).all())
        for cap_v, cap_e in ((nv - 1, ne), (nv, ne - 1)):
            a, b = ctypes.c_size_t(99), ctypes.c_size_t(99)
            hv = np.full(nv, SENTINEL, np.int64)
            hoff = np.full(nv + 1, 0x5A5A5A5A, np.uint64)
            hn, hw = np.full(ne, SENTINEL, np.int64), np.full(ne, SENTINEL, np.int64)
            assert lib.gs_slice_neighborhoods(sl.handle, hv.ctypes.data, hoff.ctypes.data, hn.ctypes.data, hw.ctypes.data,
                                              cap_v, cap_e, ctypes.byref(a), ctypes.byref(b)) == gs.GS_ERR_TRUNCATED
            assert (a.value, b.value) == (nv, ne)
            assert (hv == SENTINEL).all() and (hoff == 0x5A5A5A5A).all() and (hn == SENTINEL).all() and (hw == SENTINEL).all()
            tn = torch.full((ne,), SENTINEL, dtype=torch.int64, device=dev)
            tw = torch.full((ne,), SENTINEL, dtype=torch.int64, device=dev)
            toff = torch.full((nv + 1,), SENTINEL, dtype=torch.int64, device=dev)
            sl.wait_stream("torch")
            assert lib.gs_slice_neighborhoods_device(sl.handle, tv.data_ptr(), toff.data_ptr(), tn.data_ptr(), tw.data_ptr(),
                                                     cap_v, cap_e, ctypes.byref(a), ctypes.byref(b)) == gs.GS_ERR_TRUNCATED
            sl.sync()
            for t in (tv, toff, tn, tw):
                assert bool((t == SENTINEL).all())


# ---- 9. one handle, many windows
def test_handle_reuse_and_growth(gs):
    rng = np.random.default_rng(9)
    start = gs.hbm_bytes(0)
    with gs.Slice(edge_hint=1) as sl:
        small = gs.hbm_bytes(0)
        assert small > start
        n = 3 * T
        s = rng.integers(-50, 50, n).astype(np.int64)
        d = rng.integers(-50, 50, n).astype(np.int64)
        w = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        _check(sl, s, d, w, "out")  # growth
        assert gs.hbm_bytes(0) > small
        grown = gs.hbm_bytes(0)
        _check(sl, [9, 1, 9, 1, 4], [1, 9, 9, 4, 4], [1, 2, 3, 4, 5], "all")  # nothing stale leaks
        _check(sl, [9, 1, 9, 1, 4], [1, 9, 9, 4, 4], [1, 2, 3, 4, 5], "in")
        z = np.zeros(0, np.int64)
        _check(sl, z, z, z, "out")
        _check(sl, [3], [2], [1], "out")
        assert gs.hbm_bytes(0) == grown  # capacity is kept
    assert gs.hbm_bytes(0) == start


# ---- 10. device entry points
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_device_entry_points(gs, direction):
    import torch
    s, d, w = _multigraph()
    n = 2000
    s, d, w = s[:n], d[:n], w[:n]
    v, off, nb, wv, red = _truth(s, d, w, direction)
    with gs.Slice(edge_hint=64) as sl:
        dev = torch.device("cuda", sl.device)

        def strided(a):  # element i at index 2 i, a sentinel between
            return torch.from_numpy(np.stack([a, np.full(n, SENTINEL, np.int64)], axis=1).ravel().copy()).to(dev)

        ts, td, tw = strided(s), strided(d), strided(w)
        sl.window_device(ts, td, tw, direction, n=n, stride=2, after="torch")
        assert sl.size() == (len(v), len(nb))
        for op in OPS:
            tv = torch.full((len(v) + 1,), SENTINEL, dtype=torch.int64, device=dev)
            to = torch.full((len(v) + 1,), SENTINEL, dtype=torch.int64, device=dev)
            sl.wait_stream("torch")  # the fills run on torch's stream
            assert sl.reduce_device(op, tv, to) == len(v)
            sl.sync()
            hv, ho = tv.cpu().numpy(), to.cpu().numpy()
            assert hv[-1] == SENTINEL and ho[-1] == SENTINEL
            assert np.array_equal(hv[:-1], v) and np.array_equal(ho[:-1], red[op]), op
        tv = torch.full((len(v) + 1,), SENTINEL, dtype=torch.int64, device=dev)
        toff = torch.full((len(v) + 2,), SENTINEL, dtype=torch.int64, device=dev)
        tn = torch.full((len(nb) + 1,), SENTINEL, dtype=torch.int64, device=dev)
        tval = torch.full((len(nb) + 1,), SENTINEL, dtype=torch.int64, device=dev)
        sl.wait_stream("torch")
        assert sl.neighborhoods_device(tv, toff, tn, tval) == (len(v), len(nb))
        sl.sync()
        for t, want in ((tv, v), (toff, off.astype(np.int64)), (tn, nb), (tval, wv)):
            h = t.cpu().numpy()
            assert h[-1] == SENTINEL and np.array_equal(h[:-1], want)
        # the host forms read the same window
        gv, gr = sl.reduce("max")
        assert np.array_equal(gv, v) and np.array_equal(gr, red["max"])


# ---- 11. more tiles than one step of the tile-count scan (gsamd.TILE_SCAN_BLOCK tile counts)
@pytest.mark.parametrize("keys", ["heads-in-every-tile", "one-head-past-the-step"])
def test_tile_scan_past_one_step(gs, keys):
    """T * TILE_SCAN_BLOCK + 1 edges: the last tile's base is the sum the scan carries out of its
    first step -- every head of the window, or (src = 0 but for the last edge) the one of tile 0."""
    n = gsamd.TILE_SCAN_BLOCK * T + 1
    i = np.arange(n, dtype=np.int64)
    src = i // 3 if keys == "heads-in-every-tile" else (i == n - 1).astype(np.int64)
    val = np.random.default_rng(11).integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    v, off, nb, wv, red = _truth(src, i, val, "out")
    with gs.Slice(edge_hint=n) as sl:
        sl.window(src, i, val, "out")
        assert sl.size() == (len(v), n)
        gv, gr = sl.reduce("sum")
        assert sl.stats()["tiles"] == gsamd.TILE_SCAN_BLOCK + 1
        assert np.array_equal(gv, v) and np.array_equal(gr, red["sum"])
        gv, goff, gnb, gw = sl.neighborhoods()
        assert np.array_equal(gv, v) and np.array_equal(goff, off)
