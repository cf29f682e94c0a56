"""GPU: the triangle summary (gsamd.Triangles, the gs_triangle_* calls) against scipy on the
same edge set -- with A the symmetric 0/1 adjacency without loops, t = rowsum((A.A) o A) / 2
and T = sum(t) / 3 -- against networkx on small graphs, and against the reference's pinned
outputs (tests/golden/triangle_pins.json). Every count is an integer: comparisons are exact.
The shape cases run under every work assignment of the count step (triangle_variant)."""
import ctypes
import itertools
import json
import math
import os

import numpy as np
import pytest

import gsamd

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
SENTINEL = -0x5A5A5A5A5A5A5A5B
L = gsamd.TRIANGLE_LANES
TILE = gsamd.TRIANGLE_TILE


@pytest.fixture(params=range(gsamd.TRIANGLE_VARIANTS), ids=lambda v: "variant%d" % v)
def variant(request, gs):
    gs.testing_set("triangle_variant", request.param)
    yield request.param
    gs.testing_set("triangle_variant", None)


def _pins():
    with open(os.path.join(GOLD, "triangle_pins.json")) as f:
        return json.load(f)


def _truth(src, dst):
    """(ids ascending, t per id, T, |G|) of the graph of the edges, by the scipy expression."""
    import scipy.sparse as sp
    s = np.asarray(src, np.int64)
    d = np.asarray(dst, np.int64)
    keep = s != d
    s, d = s[keep], d[keep]
    ids = np.unique(np.concatenate([s, d]))
    n = len(ids)
    if n == 0:
        return ids, np.zeros(0, np.int64), 0, 0
    a, b = np.searchsorted(ids, s), np.searchsorted(ids, d)
    A = sp.coo_matrix((np.ones(2 * len(a), np.int64), (np.concatenate([a, b]), np.concatenate([b, a]))),
                      shape=(n, n)).tocsr()
    A.data[:] = 1
    t = np.asarray((A @ A).multiply(A).sum(axis=1)).ravel().astype(np.int64) // 2
    return ids, t, int(t.sum()) // 3, int(A.nnz) // 2


def _dev(T, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", T.device))


def _check(T, src, dst, absent=()):
    """Every answer of the handle equals the truth of the edges (src, dst)."""
    import torch
    ids, t, total, edges = _truth(src, dst)
    assert T.count() == (total, edges, len(ids))
    v, c = T.local_counts()
    assert np.array_equal(v, ids) and np.array_equal(c, t)
    v, c = T.local_counts(nonzero_only=True)
    assert np.array_equal(v, ids[t > 0]) and np.array_equal(c, t[t > 0])
    assert int(c.sum()) == 3 * total
    q = np.concatenate([ids, np.asarray(absent, np.int64)]).astype(np.int64)
    if len(q):
        tq = _dev(T, q)
        tc = torch.full((len(q) + 1,), SENTINEL, dtype=torch.int64, device=tq.device)
        tf = torch.full((len(q) + 1,), 77, dtype=torch.uint8, device=tq.device)
        T.wait_stream("torch")  # the fills above run on torch's stream
        T.find_device(tq, tc, tf, n=len(q))
        T.sync()
        hc, hf = tc.cpu().numpy(), tf.cpu().numpy()
        assert hc[-1] == SENTINEL and hf[-1] == 77
        assert np.array_equal(hc[:len(ids)], t) and np.all(hf[:len(ids)] == 1)
        assert np.all(hc[len(ids):-1] == 0) and np.all(hf[len(ids):-1] == 0)


def _clique(ids):
    e = list(itertools.combinations(ids, 2))
    return np.array([a for a, _ in e], np.int64), np.array([b for _, b in e], np.int64)


# ------------------------------------------------------------------ 1. pins
def test_window_triangles_pin(gs):
    pins = _pins()
    rows = np.array(pins["triangles_data"]["edges"], np.int64)
    ms = pins["triangles_result"]["window_ms"]
    got = []
    with gs.Triangles(edge_hint=32) as T:
        for w in np.unique(rows[:, 2] // ms):
            m = rows[:, 2] // ms == w
            got.append([T.window(rows[m, 0], rows[m, 1]), int(w) * ms + ms - 1])
    assert sorted(got) == sorted(pins["triangles_result"]["rows"]) == [[2, 399], [2, 1199], [3, 799]]
    assert sum(g[0] for g in got) == 7


def test_pin_stream_as_one_running_stream(gs):
    import networkx as nx
    rows = np.array(_pins()["triangles_data"]["edges"], np.int64)
    G = nx.Graph()
    G.add_edges_from(rows[:, :2].tolist())
    assert sum(nx.triangles(G).values()) // 3 == 9
    with gs.Triangles(edge_hint=32) as T:
        for i in range(0, len(rows), 4):
            T.fold(rows[i:i + 4, 0], rows[i:i + 4, 1])
        assert T.count() == (9, 19, 11)
        _check(T, rows[:, 0], rows[:, 1])


def test_exact_triangle_count_default_stream(gs):
    pins = _pins()
    e = np.array(pins["exact_default_stream"]["edges"], np.int64)
    want = {int(k): v for k, v in pins["exact_default_counters"]["counters"].items()}
    assert want == {-1: 4, 1: 2, 2: 2, 3: 4, 4: 1, 5: 1, 6: 2}
    for batch in (1, 2, 9):
        with gs.Triangles(edge_hint=16) as T:
            for i in range(0, len(e), batch):
                T.fold(e[i:i + batch, 0], e[i:i + batch, 1])
            v, c = T.local_counts(nonzero_only=True)
            got = dict(zip(v.tolist(), c.tolist()))
            got[-1] = T.count()[0]
            assert got == want


# ------------------------------------------------------------------ 2. degenerate input
def test_degenerate_input(gs, variant):
    with gs.Triangles(edge_hint=4) as T:
        T.fold([], [])
        assert T.count() == (0, 0, 0)
        v, c = T.local_counts()
        assert len(v) == 0 and len(c) == 0
        T.fold([5, 5, -3], [5, 5, -3])  # only self-loops: no vertex registered
        assert T.count() == (0, 0, 0)
        _check(T, [], [], absent=[5, -3])
        T.fold([7], [3])
        assert T.count() == (0, 1, 2)
        _check(T, [7], [3], absent=[5])


def test_triangle_in_every_rotation_and_flip(gs, variant):
    tri = [(1, 2), (2, 3), (3, 1)]
    for perm in itertools.permutations(tri):
        for flips in itertools.product((0, 1), repeat=3):
            e = [(b, a) if f else (a, b) for (a, b), f in zip(perm, flips)]
            e = e + e[::-1]  # each edge repeated
            with gs.Triangles(edge_hint=4) as T:
                T.fold([a for a, _ in e], [b for _, b in e])
                assert T.count() == (1, 3, 3)
                v, c = T.local_counts()
                assert v.tolist() == [1, 2, 3] and c.tolist() == [1, 1, 1]


# ------------------------------------------------------------------ 3. row-length boundaries
@pytest.mark.parametrize("n", [3, 4, 5, L - 1, L, L + 1, L + 2, 4 * L + 2])
def test_cliques(gs, variant, n):
    s, d = _clique(range(10, 10 + n))
    with gs.Triangles(edge_hint=8) as T:
        T.fold(s, d)
        assert T.count() == (math.comb(n, 3), math.comb(n, 2), n)
        v, c = T.local_counts()
        assert np.all(c == math.comb(n - 1, 2))
        _check(T, s, d)


@pytest.mark.parametrize("rim", [4, L, L + 1, 3 * L + 5])
def test_wheels(gs, variant, rim):
    r = np.arange(1, rim + 1, dtype=np.int64)
    s = np.concatenate([np.zeros(rim, np.int64), r])
    d = np.concatenate([r, np.roll(r, -1)])
    with gs.Triangles(edge_hint=8) as T:
        T.fold(s, d)
        assert T.count() == (rim, 2 * rim, rim + 1)
        v, c = T.local_counts()
        assert v[0] == 0 and c[0] == rim and np.all(c[1:] == 2)
        _check(T, s, d)


@pytest.mark.parametrize("k", [0, 1, L - 1, L, L + 1, 4 * L + 3, 5000])
def test_book_graph(gs, variant, k):
    """Two hubs joined by an edge with k common neighbours; k = 5000 has both rows beyond the
    length at which the binned count step samples the longer row in LDS."""
    w = np.arange(100, 100 + k, dtype=np.int64)
    s = np.concatenate([[1], np.full(k, 1, np.int64), np.full(k, 2, np.int64)]).astype(np.int64)
    d = np.concatenate([[2], w, w]).astype(np.int64)
    with gs.Triangles(edge_hint=8) as T:
        T.fold(s, d)
        assert T.count() == (k, 2 * k + 1, k + 2)
        _check(T, s, d)
    # the hub edge last and alone: every triangle is closed by one new edge over old rows
    with gs.Triangles(edge_hint=8) as T:
        T.fold(s[1:], d[1:])
        assert T.count()[0] == 0
        T.fold(s[:1], d[:1])
        assert T.count() == (k, 2 * k + 1, k + 2)
        _check(T, s, d)


def test_bipartite_has_long_rows_and_no_triangle(gs, variant):
    a = np.arange(0, L + 1, dtype=np.int64)
    b = np.arange(1000, 1000 + L + 1, dtype=np.int64)
    s, d = np.repeat(a, len(b)), np.tile(b, len(a))
    with gs.Triangles(edge_hint=8) as T:
        T.fold(s, d)
        assert T.count() == (0, (L + 1) ** 2, 2 * (L + 1))
        _check(T, s, d)


def test_star_with_one_rim_edge(gs, variant):
    leaves = np.arange(1, L + 2, dtype=np.int64)
    s = np.concatenate([np.zeros(L + 1, np.int64), [1]])
    d = np.concatenate([leaves, [2]])
    with gs.Triangles(edge_hint=8) as T:
        T.fold(s, d)
        assert T.count() == (1, L + 2, L + 2)
        _check(T, s, d)


# ------------------------------------------------------------------ 4. tile boundaries
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@pytest.mark.parametrize("doubled", [False, True])
def test_path_closed_at_its_end(gs, variant, n, doubled):
    """n elements: the path 0-1-...-(n-1) of n - 1 edges and, as the LAST element of the last
    tile, the edge (n-3, n-1) that closes the path's last three vertices into a triangle
    (n < 3: a path of n edges, nothing to close)."""
    if n >= 3:
        s = np.concatenate([np.arange(0, n - 1), [n - 1]]).astype(np.int64)
        d = np.concatenate([np.arange(1, n), [n - 3]]).astype(np.int64)
    else:
        s = np.arange(0, n, dtype=np.int64)
        d = s + 1
    assert len(s) == n
    if doubled:
        s, d = np.repeat(s, 2), np.repeat(d, 2)
    with gs.Triangles(edge_hint=8) as T:
        T.fold(s, d)
        assert T.count()[0] == (1 if n >= 3 else 0)
        _check(T, s, d)


# ------------------------------------------------------------------ 5. extreme ids
def test_extreme_ids(gs, variant):
    ids = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX]
    s, d = _clique(ids)
    with gs.Triangles(edge_hint=8) as T:
        T.fold(d, s)
        assert T.count() == (35, 21, 7)
        v, c = T.local_counts()
        assert v.tolist() == ids and np.all(c == 15)
        _check(T, s, d, absent=[2, I64_MAX - 2])
        T.reset()
        _check(T, [], [], absent=ids)
        T.fold(s[::-1], d[::-1])
        _check(T, s, d)


# ------------------------------------------------------------------ 6. once-only counting across folds
def _ordered_partitions(items):
    """Every ordered partition of items into non-empty blocks (13 for three items)."""
    items = list(items)
    if not items:
        yield []
        return
    for r in range(1, len(items) + 1):
        for first in itertools.combinations(items, r):
            rest = [x for x in items if x not in first]
            for tail in _ordered_partitions(rest):
                yield [list(first)] + tail


def test_one_triangle_spread_over_folds(gs, variant):
    tri = [(1, 2), (2, 3), (1, 3)]
    parts = list(_ordered_partitions(tri))
    assert len(parts) == 13
    with gs.Triangles(edge_hint=4) as T:
        for blocks in parts:
            T.reset()
            for b in blocks:
                T.fold([a for a, _ in b], [c for _, c in b])
            assert T.count() == (1, 3, 3)
            for a, b in tri:  # a later repeat of any edge adds nothing
                T.fold([b], [a])
                assert T.count() == (1, 3, 3)
            v, c = T.local_counts()
            assert v.tolist() == [1, 2, 3] and c.tolist() == [1, 1, 1]


def test_k4_one_edge_per_fold_in_every_order(gs):
    """All 720 orders of K4's six edges, one edge per fold: after every fold T and t equal
    networkx on the prefix (the truth of a prefix depends on its edge set only: cached)."""
    import networkx as nx
    edges = list(itertools.combinations(range(4), 2))
    cache = {}

    def truth(prefix):
        key = frozenset(prefix)
        if key not in cache:
            G = nx.Graph()
            G.add_edges_from(prefix)
            t = nx.triangles(G)
            cache[key] = (sum(t.values()) // 3, sorted(t.items()))
        return cache[key]

    with gs.Triangles(edge_hint=8) as T:
        for order in itertools.permutations(edges):
            T.reset()
            for i, (a, b) in enumerate(order):
                T.fold([a], [b])
                total, local = truth(order[:i + 1])
                assert T.count()[0] == total
                if i >= 2:
                    v, c = T.local_counts()
                    assert list(zip(v.tolist(), c.tolist())) == local


# ------------------------------------------------------------------ 7. batching independence
def _draws():
    rng = np.random.default_rng(0x7A1A)
    s = rng.integers(0, 200, 3000)
    d = rng.integers(0, 200, 3000)
    d[::97] = s[::97]  # loops
    mult = np.uint64(0x9E3779B97F4A7C15)
    scr = lambda x: (x.astype(np.uint64) * mult).view(np.int64)  # ids scrambled to 64 bits
    return scr(s), scr(d)


def test_batching_independence(gs, variant):
    s, d = _draws()
    pairs = np.stack([np.minimum(s, d), np.maximum(s, d)], axis=1)
    assert np.any(s == d) and len(np.unique(pairs, axis=0)) < len(s)  # loops and repeats are in
    rng = np.random.default_rng(5)
    with gs.Triangles(edge_hint=64) as T:
        T.fold(s, d)
        _check(T, s, d)
        T.reset()
        i = 0
        while i < len(s):
            c = int(rng.integers(1, 400))
            T.fold(s[i:i + c], d[i:i + c])
            i += c
        _check(T, s, d)
        T.reset()
        T.fold(d[::-1], s[::-1])
        _check(T, s, d)
        T.fold(s, d)  # the stream twice
        _check(T, s, d)
        T.reset()
        for i in range(300):
            T.fold(s[i:i + 1], d[i:i + 1])
        _check(T, s[:300], d[:300])


# ------------------------------------------------------------------ 8. growth
def test_growth_from_a_tiny_hint_and_hbm_accounting(gs, variant):
    start = gs.hbm_bytes(0)
    rng = np.random.default_rng(11)
    s = rng.integers(0, 1 << 12, 1 << 14)
    d = rng.integers(0, 1 << 12, 1 << 14)
    with gs.Triangles(edge_hint=1) as T:
        small = gs.hbm_bytes(0)
        assert small > start
        for i in range(0, len(s), 1 << 12):
            T.fold(s[i:i + (1 << 12)], d[i:i + (1 << 12)])
            _check(T, s[:i + (1 << 12)], d[:i + (1 << 12)])
        assert gs.hbm_bytes(0) > small
    assert gs.hbm_bytes(0) == start


# ------------------------------------------------------------------ 9. device entry points
def test_device_entry_points(gs, variant):
    import torch
    s, d = _draws()
    s, d = s[:1000], d[:1000]
    ids, t, total, edges = _truth(s, d)
    with gs.Triangles(edge_hint=64) as T:
        dev = torch.device("cuda", T.device)
        pairs = _dev(T, np.stack([s[:500], d[:500]], axis=1)).contiguous().view(-1)
        T.fold_device(pairs, pairs[1:], n=500, stride=2, after="torch")
        ts, td = _dev(T, s[500:]), _dev(T, d[500:])  # written on torch's stream
        T.fold_device(ts, td, after="torch")
        out = torch.full((4,), SENTINEL, dtype=torch.int64, device=dev)
        T.wait_stream("torch")  # the fill runs on torch's stream
        T.count_device(out)
        T.sync()
        assert out.cpu().numpy().tolist() == [total, edges, len(ids), SENTINEL]
        _check(T, s, d, absent=[12345, I64_MIN])
        for nz in (False, True):
            want_v = ids[t > 0] if nz else ids
            want_c = t[t > 0] if nz else t
            tv = torch.full((len(want_v) + 1,), SENTINEL, dtype=torch.int64, device=dev)
            tc = torch.full((len(want_v) + 1,), SENTINEL, dtype=torch.int64, device=dev)
            T.wait_stream("torch")
            assert T.local_counts_device(tv, tc, nonzero_only=nz) == len(want_v)
            hv, hc = tv.cpu().numpy(), tc.cpu().numpy()
            assert hv[-1] == SENTINEL and hc[-1] == SENTINEL
            assert np.array_equal(hv[:-1], want_v) and np.array_equal(hc[:-1], want_c)
        # truncation: *n set, nothing written
        lib = gs.lib()
        got = ctypes.c_size_t(99)
        tv = torch.full((len(ids),), SENTINEL, dtype=torch.int64, device=dev)
        tc = torch.full((len(ids),), SENTINEL, dtype=torch.int64, device=dev)
        T.wait_stream("torch")
        assert lib.gs_triangle_export_device(T.handle, tv.data_ptr(), tc.data_ptr(), len(ids) - 1, ctypes.byref(got),
                                             0) == gs.GS_ERR_TRUNCATED
        assert got.value == len(ids)
        hv = np.full(len(ids), SENTINEL, np.int64)
        hc = np.full(len(ids), SENTINEL, np.int64)
        got.value = 99
        assert lib.gs_triangle_export(T.handle, hv.ctypes.data, hc.ctypes.data, len(ids) - 1, ctypes.byref(got),
                                      0) == gs.GS_ERR_TRUNCATED
        assert got.value == len(ids) and np.all(hv == SENTINEL) and np.all(hc == SENTINEL)
        T.sync()
        assert np.all(tv.cpu().numpy() == SENTINEL) and np.all(tc.cpu().numpy() == SENTINEL)
        assert T.stream


# ------------------------------------------------------------------ 10. reset and window
def test_reset_and_windows(gs, variant):
    s, d = _draws()
    with gs.Triangles(edge_hint=64) as T:
        T.fold(s[:800], d[:800])
        ids = _truth(s[:800], d[:800])[0]
        T.reset()
        assert T.count() == (0, 0, 0)
        v, c = T.local_counts()
        assert len(v) == 0
        _check(T, [], [], absent=ids[:50])
        for i in range(0, 3000, 600):
            assert T.window(s[i:i + 600], d[i:i + 600]) == _truth(s[i:i + 600], d[i:i + 600])[2]
            _check(T, s[i:i + 600], d[i:i + 600])
