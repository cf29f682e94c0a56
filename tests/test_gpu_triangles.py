"""GPU: the triangle summary (gsamd.Triangles, the gs_triangle_* calls) against scipy on the
same edge set -- with A the symmetric 0/1 adjacency without loops, t = rowsum((A.A) o A) / 2
and T = sum(t) / 3 -- against networkx on small graphs, and against the reference's pinned
outputs (tests/golden/triangle_pins.json). Every count is an integer: comparisons are exact.
The shape cases run under every work assignment of the count step (triangle_variant).
Section 11 fills every bin of the product's assignment at its thresholds and checks the
assignment itself (the list lengths, the step count, the longest row) against a host model."""
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
SHORT_ROW = gsamd.TRIANGLE_SHORT_ROW
WAVE_ROW = gsamd.TRIANGLE_WAVE_ROW
LDS_ROW = gsamd.TRIANGLE_LDS_ROW


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


_TRUTHS = {}


def _shared_truth(key, src, dst):
    """_truth of a graph that several cases (the variants, the fold orders) share, computed once."""
    if key not in _TRUTHS:
        _TRUTHS[key] = _truth(src, dst)
    return _TRUTHS[key]


def _assignment(folds):
    """Host model of the product's work assignment for the folds [(src, dst), ...] applied after
    a reset: ([(short, wave, workgroup) per fold], steps, hot). A fold's new edges are its
    canonical pairs that are no loop, no repeat and in no earlier fold; k_tri_rows reads the
    rows of the adjacency the fold was merged into, so slen / llen of a new edge are the smaller
    / larger degree of its endpoints AFTER the fold. steps is the sum of slen and hot the
    greatest llen over every new edge so far."""
    folds = [(np.asarray(s, np.int64), np.asarray(d, np.int64)) for s, d in folds]
    ids = np.unique(np.concatenate([np.zeros(0, np.int64)] + [a for f in folds for a in f]))
    n = max(len(ids), 1)
    deg = np.zeros(n, np.int64)
    seen = np.zeros(0, np.int64)
    per_fold, steps, hot = [], 0, 0
    for s, d in folds:
        a, b = np.searchsorted(ids, s), np.searchsorted(ids, d)
        keep = a != b
        new = np.setdiff1d(np.minimum(a, b)[keep] * n + np.maximum(a, b)[keep], seen)  # sorted, unique
        seen = np.concatenate([seen, new])
        lo, hi = new // n, new % n
        deg += np.bincount(lo, minlength=n) + np.bincount(hi, minlength=n)
        slen, llen = np.minimum(deg[lo], deg[hi]), np.maximum(deg[lo], deg[hi])
        workgroup = int(np.sum((slen > WAVE_ROW) & (llen >= LDS_ROW)))
        wave = int(np.sum(slen > SHORT_ROW)) - workgroup
        per_fold.append((len(new) - wave - workgroup, wave, workgroup))
        steps += int(slen.sum())
        hot = max(hot, int(llen.max()) if len(new) else 0)
    return per_fold, steps, hot


def _check_assignment(T, folds, variant):
    """After the last of the folds: the library's step count and longest row equal the model's
    under every variant, and the lengths of the product's wave and workgroup lists equal the
    model's for the last fold that had new edges (variant 1 keeps no lists)."""
    per_fold, steps, hot = _assignment(folds)
    st = T.stats()
    assert (st["steps"], st["hot_row"]) == (steps, hot)
    last = [f for f in per_fold if sum(f)]
    want = last[-1][1:] if last and variant == 0 else (0, 0)
    assert T.bins() == want
    return per_fold


def _dev(T, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", T.device))


def _check(T, src, dst, absent=(), truth=None):
    """Every answer of the handle equals the truth of the edges (src, dst); truth: _truth(src,
    dst) where the caller holds it already."""
    import torch
    ids, t, total, edges = truth if truth is not None else _truth(src, dst)
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


# ------------------------------------------------------------------ 11. every bin of the count step
# The product's count step gives a new edge to a lane group (shorter row <= SHORT_ROW), to a
# workgroup that samples the longer row in LDS (shorter row > WAVE_ROW and longer row >=
# LDS_ROW) or to a wave (the rest). Every case below states in literal numbers, on the host
# model and before it touches the GPU, which bins it fills: after a retune of a threshold
# the case fails instead of testing another kernel than it names.
_NB0 = 1000  # the smallest neighbour of the hub of _hub_and_clique
WAYS = ("one_fold", "hub_first", "hub_last")


def _hub_and_clique(c, D, where):
    """A hub with the D neighbours _NB0, _NB0 + 2, ...; c of them, the mids, form a clique and
    the others are leaves, so that an edge (hub, mid) has a shorter row of c and a longer row of
    D entries. The mids are every 61st neighbour and the last one: they fall into many sample
    segments of the hub's row, the first and the last among them. where: the hub's id below
    every other id (its triangles are counted at the mid-mid edges), above every other id
    (counted at the hub's edges) or inside the mids' range (either, per triangle).
    Returns (hub, mids, the hub's edges, the clique's edges)."""
    nb = _NB0 + 2 * np.arange(D, dtype=np.int64)
    pos = np.concatenate([61 * np.arange(c - 1), [D - 1]])
    assert np.all(np.diff(pos) > 0)
    mids = nb[pos]
    hub = {"below": 5, "above": _NB0 + 2 * D + 5000, "middle": int(mids[c // 2]) + 1}[where]
    hs, hd = np.full(D, hub, np.int64), nb.copy()
    hs[1::2], hd[1::2] = hd[1::2].copy(), hs[1::2].copy()  # both directions occur
    return hub, mids, (hs, hd), _clique(mids.tolist())


def _in_ways(hub_edges, other_edges):
    both = tuple(np.concatenate([a, b]) for a, b in zip(hub_edges, other_edges))
    return {"one_fold": [both], "hub_first": [hub_edges, other_edges], "hub_last": [other_edges, hub_edges]}


def _fold_and_check(gs, variant, folds, truth):
    s = np.concatenate([f[0] for f in folds])
    d = np.concatenate([f[1] for f in folds])
    with gs.Triangles(edge_hint=64) as T:
        for k, (fs, fd) in enumerate(folds):
            T.fold(fs, fd)
            _check_assignment(T, folds[:k + 1], variant)
        _check(T, s, d, truth=truth)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("where", ["below", "above", "middle"])
@pytest.mark.parametrize("D", [4095, 4096, 4097, 4101, 5120, 5121])
@pytest.mark.parametrize("c", [64, 65])
def test_hub_and_clique_at_the_thresholds(gs, variant, c, D, where, way):
    """Both thresholds of the workgroup bin bracketed: a shorter row of 64 | 65 against a longer
    row of 4095 | 4096 | 4097 entries; further 4096 and 5120 (exactly 1024 samples), 4097 and
    5121 (the sample step goes from 4 to 5 and from 5 to 6, a last segment of 2 and of 3
    entries) and 4101 (a last segment of one entry). In one fold all three edges of a triangle
    are new; with the hub's edges in a fold of their own, first or last, the rows of the walk
    mix entries of the fold with older ones."""
    hub, mids, hub_edges, clique_edges = _hub_and_clique(c, D, where)
    folds = _in_ways(hub_edges, clique_edges)[way]
    per_fold, steps, hot = _assignment(folds)
    pairs = math.comb(c, 2)
    sampled = c == 65 and D >= 4096  # the c edges (hub, mid) take a workgroup each
    of_hub = (D - c, 0, c) if sampled else (D - c, c, 0)
    assert per_fold == {"one_fold": [(D - c, pairs + of_hub[1], of_hub[2])],
                        "hub_first": [(D, 0, 0), (0, pairs, 0)],
                        "hub_last": [(0, pairs, 0), of_hub]}[way]
    assert hot == D
    assert steps == {"one_fold": pairs * c + c * c + D - c, "hub_first": D + pairs * c,
                     "hub_last": pairs * (c - 1) + c * c + D - c}[way]
    if sampled:
        assert gs.TRIANGLE_SAMPLES == 1024  # the sample arithmetic these lengths were chosen for
        step = -(-D // 1024)
        nsamp = -(-D // step)
        assert (step, nsamp, D - (nsamp - 1) * step) == {4096: (4, 1024, 4), 4097: (5, 820, 2), 4101: (5, 821, 1),
                                                         5120: (5, 1024, 5), 5121: (6, 854, 3)}[D]
    s = np.concatenate([hub_edges[0], clique_edges[0]])
    d = np.concatenate([hub_edges[1], clique_edges[1]])
    truth = _shared_truth(("hub and clique", c, D, where), s, d)
    ids, t, total, edges = truth
    assert total == pairs + math.comb(c, 3) and edges == D + pairs and len(ids) == D + 1
    assert t[ids == hub].tolist() == [pairs] and np.all(t[np.isin(ids, mids)] == c - 1 + math.comb(c - 1, 2))
    assert int(t.sum()) == pairs + c * (c - 1 + math.comb(c - 1, 2))  # the leaves have none
    _fold_and_check(gs, variant, folds, truth)


@pytest.mark.parametrize("way", ["one_fold", "hub_last"])
@pytest.mark.parametrize("where", ["below", "above", "middle"])
def test_neighbours_the_sampled_search_rejects(gs, variant, where, way):
    """The hub and clique with 65 mids and 4097 neighbours (sample step 5, a last segment of two
    entries), where four mids (the first and the last neighbour of the hub among them) have
    three more neighbours each that the hub has not: one below the hub's first neighbour (no
    sample is <= it), one above its last, one strictly between two consecutive neighbours of
    the same sample segment. They are vertices without a triangle, and no count changes."""
    c, D, step = 65, 4097, 5
    hub, mids, hub_edges, clique_edges = _hub_and_clique(c, D, where)
    owners = mids[[0, 21, 42, 64]]
    inside = np.array([7, 2001, 3001, 4095])  # neighbours p and p + 1 lie in one segment
    assert -(-D // 1024) == step and np.all(inside % step != step - 1) and inside.max() + 1 == D - 1
    extras = np.concatenate([100 + np.arange(4), _NB0 + 2 * D + 100 + np.arange(4), _NB0 + 2 * inside + 1])
    assert hub not in extras and len(np.unique(extras)) == 12
    other = (np.concatenate([clique_edges[0], extras]), np.concatenate([clique_edges[1], np.tile(owners, 3)]))
    folds = _in_ways(hub_edges, other)[way]
    per_fold, steps, hot = _assignment(folds)
    pairs = math.comb(c, 2)
    assert per_fold == {"one_fold": [(D - c + 12, pairs, c)], "hub_last": [(12, pairs, 0), (D - c, 0, c)]}[way]
    assert hot == D
    s = np.concatenate([hub_edges[0], other[0]])
    d = np.concatenate([hub_edges[1], other[1]])
    truth = _shared_truth(("rejected neighbours", where), s, d)
    ids, t, total, edges = truth
    assert total == pairs + math.comb(c, 3) and edges == D + pairs + 12 and len(ids) == D + 13
    assert np.all(t[np.isin(ids, extras)] == 0) and t[ids == hub].tolist() == [pairs]
    _fold_and_check(gs, variant, folds, truth)


def test_more_workgroup_edges_than_workgroups(gs, variant):
    """One fold with 1176 edges in the workgroup list, which 1024 workgroups serve: some take a
    second edge. 16 hubs in a clique, 66 mids in a clique and 4030 leaves, every mid and every
    leaf adjacent to every hub; the hubs have the greatest ids, so their edges count."""
    leaves = 1000 + 2 * np.arange(4030, dtype=np.int64)
    mids = 1001 + 2 * 61 * np.arange(66, dtype=np.int64)  # among the leaves
    hubs = 100000 + np.arange(16, dtype=np.int64)
    assert mids.max() < leaves.max()
    parts = [_clique(hubs.tolist()), _clique(mids.tolist()), (np.repeat(hubs, 66), np.tile(mids, 16)),
             (np.tile(leaves, 16), np.repeat(hubs, 4030))]
    s = np.concatenate([p[0] for p in parts])
    d = np.concatenate([p[1] for p in parts])
    order = np.random.default_rng(12).permutation(len(s))
    s, d = s[order], d[order]
    assert len(s) == 67801
    per_fold, steps, hot = _assignment([(s, d)])
    assert per_fold == [(16 * 4030, math.comb(66, 2), math.comb(16, 2) + 16 * 66)]
    assert per_fold[0][2] == 1176 > 1024 and hot == 15 + 66 + 4030
    assert steps == 16 * 4030 * 16 + (math.comb(66, 2) + 16 * 66) * 81 + math.comb(16, 2) * 4111
    truth = _shared_truth("sixteen hubs", s, d)
    assert truth[2] == math.comb(16, 3) + math.comb(66, 3) + math.comb(16, 2) * 4096 + 16 * math.comb(66, 2) == 572160
    _fold_and_check(gs, variant, [(s, d)], truth)


def test_more_wave_edges_than_the_wave_grid_takes_at_once(gs, variant):
    """One fold with more than 16384 edges in the wave list (4096 workgroups of 4 edges: a second
    iteration), every shorter row above 64 entries and no row near 4096: G(640, 0.15)."""
    iu = np.triu_indices(640, 1)
    m = np.random.default_rng(3).random(len(iu[0])) < 0.15
    s, d = iu[0][m].astype(np.int64), iu[1][m].astype(np.int64)
    per_fold, steps, hot = _assignment([(s, d)])
    short, wave, workgroup = per_fold[0]
    assert wave > 16384 and workgroup == 0 and short == 0 and wave == len(s)
    assert 64 < np.bincount(np.concatenate([s, d])).min() and hot < 4096
    _fold_and_check(gs, variant, [(s, d)], _shared_truth("G(640, 0.15)", s, d))


@pytest.mark.parametrize("repeat", ["thrice", "one_to_three"])
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 5])
def test_repeats_and_loops_at_every_thread_and_tile_edge(gs, variant, n, repeat):
    """The stream of test_path_closed_at_its_end with every edge three times, or edge i
    1 + i % 3 times, and a self-loop after every seventh element: in the sorted fold the runs
    of equal pairs start at every position of a thread's four elements and lie across the
    edges of the tiles. Folded twice: the second fold has no new edge."""
    s = np.concatenate([np.arange(0, n - 1), [n - 1]]).astype(np.int64)
    d = np.concatenate([np.arange(1, n), [n - 3]]).astype(np.int64)
    reps = np.full(n, 3) if repeat == "thrice" else 1 + np.arange(n) % 3
    s, d = np.repeat(s, reps), np.repeat(d, reps)
    at = np.arange(7, len(s) + 1, 7)
    loops = s[at - 1]
    s, d = np.insert(s, at, loops), np.insert(d, at, loops)
    assert len(s) == int(reps.sum()) + len(at) and np.sum(s == d) == len(at) > 100
    # the sorted fold as k_tri_flag_new reads it: where the runs of equal pairs start and what they straddle
    lo, hi = np.minimum(s, d), np.maximum(s, d)
    o = np.lexsort((hi, lo))
    lo, hi = lo[o], hi[o]
    same = (lo[1:] == lo[:-1]) & (hi[1:] == hi[:-1])  # same[i]: elements i and i + 1 are equal
    starts = np.flatnonzero(same & ~np.concatenate([[False], same[:-1]]))
    assert set((starts % 4).tolist()) == {0, 1, 2, 3}
    assert np.any(same[3::4])  # a run goes on from one thread's last element to the next thread's first
    assert np.any(same[TILE - 1::TILE])  # and from one tile's last element to the next tile's first
    per_fold, steps, hot = _assignment([(s, d), (s, d)])
    assert per_fold == [(n, 0, 0), (0, 0, 0)] and hot == 3
    truth = _shared_truth(("closed path", n), s, d)
    assert truth[2:] == (1, n) and len(truth[0]) == n
    with gs.Triangles(edge_hint=8) as T:
        T.fold(s, d)
        assert T.count() == (1, n, n)
        _check(T, s, d, truth=truth)
        _check_assignment(T, [(s, d)], variant)
        T.fold(s, d)
        assert T.count() == (1, n, n) and T.bins() == (0, 0)
        _check(T, s, d, truth=truth)
        _check_assignment(T, [(s, d), (s, d)], variant)


_STREAM = []


def _hub_and_core_stream():
    """47 K elements over 5000 vertices, shuffled, ids scrambled to 64 bits: 30000 uniform pairs
    (loops and repeats among them), a core of 100 vertices with p = 0.8, three core vertices
    joined to 4500 vertices each."""
    if not _STREAM:
        rng = np.random.default_rng(0x7A1B)
        nv = 5000
        core = rng.choice(nv, 100, replace=False)
        iu = np.triu_indices(100, 1)
        m = rng.random(len(iu[0])) < 0.8
        s = [rng.integers(0, nv, 30000), core[iu[0][m]]]
        d = [rng.integers(0, nv, 30000), core[iu[1][m]]]
        for h in core[:3]:
            s.append(np.full(4500, h))
            d.append(rng.choice(nv, 4500, replace=False))
        s, d = np.concatenate(s), np.concatenate(d)
        order = rng.permutation(len(s))
        mult = np.uint64(0x9E3779B97F4A7C15)
        for a in (s, d):
            a = (a[order].astype(np.uint64) * mult).view(np.int64)
            a.setflags(write=False)
            _STREAM.append(a)
    return _STREAM


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_hub_and_core_stream_in_three_folds(gs, variant, order):
    """A random stream whose last fold fills all three bins, checked after every fold, with
    its three parts in either order."""
    s, d = _hub_and_core_stream()
    k = len(s) // 3
    parts = [(s[:k], d[:k]), (s[k:2 * k], d[k:2 * k]), (s[2 * k:], d[2 * k:])]
    if order == "reverse":
        parts = parts[::-1]
    per_fold, steps, hot = _assignment(parts)
    assert min(per_fold[-1]) > 0 and hot >= 4096
    with gs.Triangles(edge_hint=64) as T:
        for i in range(3):
            T.fold(*parts[i])
            cs = np.concatenate([p[0] for p in parts[:i + 1]])
            cd = np.concatenate([p[1] for p in parts[:i + 1]])
            _check(T, cs, cd, truth=_shared_truth(("hub and core", order, i), cs, cd))
            _check_assignment(T, parts[:i + 1], variant)


# ---- 12. more tiles than one step (new edges) and two steps (export) of the tile-count scan
def test_tile_scan_past_its_steps(gs):
    """TILE * TILE_SCAN_BLOCK + 2 edges forming disjoint triangles, in one fold: the dedup scans
    one tile count more than a step of gsamd.TILE_SCAN_BLOCK, the export of the 2 |G| adjacency
    entries one more than two steps. T = the number of triangles, t(v) = 1 for every vertex, and
    folding the same edges again adds nothing."""
    n = gsamd.TILE_SCAN_BLOCK * TILE + 2
    assert n % 3 == 0 and -(-n // TILE) == gsamd.TILE_SCAN_BLOCK + 1 and -(-2 * n // TILE) == 2 * gsamd.TILE_SCAN_BLOCK + 1
    k = 3 * np.arange(n // 3, dtype=np.int64)
    src = np.stack([k, k + 1, k], axis=1).ravel()
    dst = np.stack([k + 1, k + 2, k + 2], axis=1).ravel()
    with gs.Triangles(edge_hint=n) as T:
        for fold in range(2):
            T.fold(src, dst)
            assert T.count() == (n // 3, n, n), fold
            v, c = T.local_counts()
            assert np.array_equal(v, np.arange(n, dtype=np.int64)) and bool((c == 1).all()), fold
