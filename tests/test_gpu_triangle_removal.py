"""GPU: edges leave the triangle summary (gsamd.SlidingTriangles.remove / remove_device / expire /
slide). After every call the handle must equal a fresh handle that folded exactly the surviving
edge set: the truth is the scipy expression of test_gpu_triangles.py on that set (with A the
symmetric 0/1 adjacency without loops, t = rowsum((A.A) o A) / 2 and T = sum(t) / 3), and every
comparison is exact. The check reads count, both exports and find_device, `found` on vanished
and never-seen ids included. Shape cases run under both work assignments of the count step."""
import itertools

import numpy as np
import pytest

import gsamd

pytestmark = pytest.mark.gpu

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
SENTINEL = -0x5A5A5A5A5A5A5A5B
TILE = gsamd.TRIANGLE_TILE
SHORT_ROW = gsamd.TRIANGLE_SHORT_ROW
WAVE_ROW = gsamd.TRIANGLE_WAVE_ROW
LDS_ROW = gsamd.TRIANGLE_LDS_ROW
MULT = np.uint64(0x9E3779B97F4A7C15)


@pytest.fixture(params=range(gsamd.TRIANGLE_VARIANTS), ids=lambda v: "variant%d" % v)
def variant(request, gs):
    gs.testing_set("triangle_variant", request.param)
    yield request.param
    gs.testing_set("triangle_variant", None)


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
    """Every answer of the handle equals the truth of the edges (src, dst); `absent`: ids that are
    no vertex of it (vanished or never seen). Returns the truth."""
    import torch
    ids, t, total, edges = truth = _truth(src, dst)
    assert T.count() == (total, edges, len(ids))
    v, c = T.local_counts()
    assert np.array_equal(v, ids) and np.array_equal(c, t)
    v, c = T.local_counts(nonzero_only=True)
    assert np.array_equal(v, ids[t > 0]) and np.array_equal(c, t[t > 0])
    assert int(c.sum()) == 3 * total
    absent = np.setdiff1d(np.asarray(absent, np.int64), ids)
    q = np.concatenate([ids, absent]).astype(np.int64)
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
    return truth


class _Model:
    """The surviving pairs with their stamps, on the host: what the contract says G is."""

    def __init__(self, refresh=False):
        self.stamp = {}
        self.fold_no = 0
        self.refresh = refresh

    @staticmethod
    def _pairs(src, dst):
        return [(min(a, b), max(a, b)) for a, b in zip(np.asarray(src, np.int64).tolist(),
                                                      np.asarray(dst, np.int64).tolist()) if a != b]

    def fold(self, src, dst):
        self.fold_no += 1
        for p in self._pairs(src, dst):
            if self.refresh or p not in self.stamp:
                self.stamp[p] = self.fold_no

    def remove(self, src, dst):
        for p in self._pairs(src, dst):
            self.stamp.pop(p, None)

    def expire(self, folds):
        self.stamp = {p: s for p, s in self.stamp.items() if s + folds > self.fold_no}

    def edges(self):
        p = sorted(self.stamp)
        return np.array([a for a, _ in p], np.int64), np.array([b for _, b in p], np.int64)


def _clique(ids):
    e = list(itertools.combinations(ids, 2))
    return np.array([a for a, _ in e], np.int64), np.array([b for _, b in e], np.int64)


def _without(src, dst, rs, rd):
    """The edges (src, dst) that are none of the unordered pairs (rs, rd)."""
    dead = set(_Model._pairs(rs, rd))
    keep = np.array([(min(a, b), max(a, b)) not in dead for a, b in zip(src.tolist(), dst.tolist())], bool)
    return src[keep], dst[keep]


# ------------------------------------------------------------------ 1. the once-only rule, exhaustively
def _every_subset(gs, s, d, subsets):
    """Fold (s, d), remove the subset in ONE call, check; a triangle that loses one, two or three
    edges must be taken away exactly once."""
    every = np.unique(np.concatenate([s, d]))
    with gs.SlidingTriangles(edge_hint=16) as T:
        for sub in subsets:
            T.reset()
            T.fold(s, d)
            idx = np.array(sub, np.int64)
            rs, rd = s[idx], d[idx]
            if len(idx) % 2:
                rs, rd = rd, rs  # a removal names unordered pairs
            T.remove(rs, rd)
            keep = np.setdiff1d(np.arange(len(s)), idx)
            ids, t, total, edges = _check(T, s[keep], d[keep], absent=every)
            st = T.remove_stats()
            assert st["edges_removed"] == len(idx) and st["entries"] == 2 * edges
            assert st["vertices_vanished"] == len(every) - len(ids)


def _subsets(m):
    return [c for k in range(m + 1) for c in itertools.combinations(range(m), k)]


def test_k4_every_subset_of_its_edges(gs, variant):
    s, d = _clique([3, 5, 8, 13])
    assert len(_subsets(6)) == 64
    _every_subset(gs, s, d, _subsets(6))


def test_k3_with_a_pendant_vertex_every_subset(gs, variant):
    s = np.array([10, 20, 10, 30], np.int64)
    d = np.array([20, 30, 30, 40], np.int64)
    _every_subset(gs, s, d, _subsets(4))


def test_k5_every_subset_of_its_edges(gs):
    s, d = _clique([-7, 0, 4, 9, 1 << 40])
    assert len(_subsets(10)) == 1024
    _every_subset(gs, s, d, _subsets(10))


# ------------------------------------------------------------------ 2. what changes nothing
def test_removals_that_change_nothing(gs, variant):
    s, d = _clique([1, 2, 3, 4, 5])
    with gs.SlidingTriangles(edge_hint=16) as T:
        T.remove(np.array([1, 2], np.int64), np.array([2, 3], np.int64))  # an empty handle
        T.remove(np.zeros(0, np.int64), np.zeros(0, np.int64))
        assert T.count() == (0, 0, 0) and T.remove_stats()["edges_removed"] == 0
        T.fold(s, d)
        T.remove(np.array([1, 7, 8, 5], np.int64), np.array([9, 8, 1, 6], np.int64))  # pairs not in G
        _check(T, s, d, absent=[6, 7, 8, 9])
        T.remove(np.array([1, 2, 3], np.int64), np.array([1, 2, 3], np.int64))  # loops
        _check(T, s, d)
        T.remove(np.zeros(0, np.int64), np.zeros(0, np.int64))
        _check(T, s, d)
        assert T.remove_stats()["edges_removed"] == 0 and T.remove_stats()["triangles_destroyed"] == 0
        # one pair five times, in both directions, among loops and absent pairs: it leaves once
        T.remove(np.array([2, 4, 2, 9, 4, 4, 2, 4], np.int64), np.array([4, 2, 4, 9, 2, 4, 4, 77], np.int64))
        ks, kd = _without(s, d, np.array([2], np.int64), np.array([4], np.int64))
        _check(T, ks, kd, absent=[9, 77])
        st = T.remove_stats()
        assert (st["edges_removed"], st["triangles_destroyed"], st["vertices_vanished"]) == (1, 3, 0)
        T.remove(np.array([4], np.int64), np.array([2], np.int64))  # gone already
        _check(T, ks, kd)


# ------------------------------------------------------------------ 3. vanish and return
@pytest.mark.parametrize("v", [6, I64_MIN, I64_MAX], ids=["plain", "int64_min", "int64_max"])
def test_a_vertex_vanishes_and_returns(gs, variant, v):
    ids = [1, 2, 3, 4, 5, v]
    s, d = _clique(ids)
    mine = (s == v) | (d == v)
    with gs.SlidingTriangles(edge_hint=16) as T:
        T.fold(s, d)
        _check(T, s, d)
        T.remove(d[mine], s[mine])  # every edge of v
        _check(T, s[~mine], d[~mine], absent=[v])
        st = T.remove_stats()
        assert (st["edges_removed"], st["triangles_destroyed"], st["vertices_vanished"]) == (5, 10, 1)
        T.fold(np.array([v, 2], np.int64), np.array([1, v], np.int64))  # v is a new vertex again
        ks = np.concatenate([s[~mine], [v, 2]])
        kd = np.concatenate([d[~mine], [1, v]])
        ids2, t2, _, _ = _check(T, ks, kd)
        assert t2[ids2 == v].tolist() == [1]


def test_remove_all_of_g_then_fold_again(gs, variant):
    s, d = _clique([I64_MIN, -3, 0, 11, I64_MAX])
    with gs.SlidingTriangles(edge_hint=16) as T:
        T.fold(s, d)
        T.remove(s, d)
        assert T.count() == (0, 0, 0)
        for nz in (False, True):
            v, c = T.local_counts(nonzero_only=nz)
            assert len(v) == 0 and len(c) == 0
        _check(T, s[:0], d[:0], absent=np.unique(np.concatenate([s, d])))
        assert T.remove_stats()["vertices_vanished"] == 5 and T.remove_stats()["entries"] == 0
        T.fold(s[2:], d[2:])
        _check(T, s[2:], d[2:])
        T.fold(s, d)
        _check(T, s, d)


# ------------------------------------------------------------------ 4. tiles
def _path_with_apex():
    """A path 0 - 1 - ... - n-1 of more than 2 TILE + 1 edges and an apex above every id that
    closes a triangle over the path edges (0, 1), (300, 301) and (n-2, n-1). A's rows are the
    vertices in order, two entries per inner vertex: removing consecutive path edges kills runs
    of consecutive entries, broken only where an apex entry survives."""
    n = 2 * TILE + 300
    apex = n + 10
    at = np.array([0, 1, 300, 301, n - 2, n - 1], np.int64)
    s = np.concatenate([np.arange(n - 1, dtype=np.int64), np.full(len(at), apex, np.int64)])
    d = np.concatenate([np.arange(1, n, dtype=np.int64), at])
    return n, apex, s, d


@pytest.mark.parametrize("end", ["head", "tail"])
@pytest.mark.parametrize("k", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_runs_of_dying_entries_across_tiles(gs, variant, k, end):
    """k removed edges (the dedup's tiles) whose entries form runs that straddle the tile
    boundaries of A (more than 4 TILE entries); the run of the largest k covers whole tiles. The
    head case kills A's first entry (0, 1), the tail case its last one (apex, n-1)."""
    n, apex, s, d = _path_with_apex()
    assert 2 * len(s) > 2 * TILE and k < n - 1
    if end == "head":
        rs, rd = np.arange(k, dtype=np.int64), np.arange(1, k + 1, dtype=np.int64)
    else:
        rs = np.concatenate([np.arange(n - k, n, dtype=np.int64)[:-1], [apex]])
        rd = np.concatenate([np.arange(n - k - 1, n - 1, dtype=np.int64)[:-1], [n - 1]])
    assert len(rs) == k
    rng = np.random.default_rng(k)
    order = rng.permutation(k)
    with gs.SlidingTriangles(edge_hint=64) as T:
        T.fold(s, d)
        T.remove(rs[order], rd[order])
        ks, kd = _without(s, d, rs, rd)
        ids, t, total, edges = _check(T, ks, kd, absent=np.arange(n))
        st = T.remove_stats()
        assert st["edges_removed"] == k and st["entries"] == 2 * edges
        assert st["vertices_vanished"] == n + 1 - len(ids) and st["vertices_vanished"] >= k - 4
        assert st["triangles_destroyed"] == 3 - total


# ------------------------------------------------------------------ 5. bins
_NB0 = 1000


def _hub_and_clique(c, D):
    """test_gpu_triangles.py's graph: a hub above every id with the D neighbours _NB0, _NB0 + 2,
    ...; c of them (every 61st and the last) form a clique, the others are leaves. An edge (hub,
    mid) has a shorter row of c and a longer row of D entries, an edge (mid, mid) two rows of c,
    an edge (hub, leaf) a shorter row of one."""
    nb = _NB0 + 2 * np.arange(D, dtype=np.int64)
    pos = np.concatenate([61 * np.arange(c - 1), [D - 1]])
    mids = nb[pos]
    hub = _NB0 + 2 * D + 5000
    leaves = np.setdiff1d(nb, mids)
    hs, hd = np.full(D, hub, np.int64), nb.copy()
    hs[1::2], hd[1::2] = hd[1::2].copy(), hs[1::2].copy()
    cs, cd = _clique(mids.tolist())
    return hub, mids, leaves, np.concatenate([hs, cs]), np.concatenate([hd, cd])


def _removal_model(s, d, rs, rd):
    """(wave list, workgroup list, steps) of the removal of the distinct pairs (rs, rd), all in
    the loop-free, repeat-free graph (s, d): the rows are those BEFORE the removal."""
    ids, cnt = np.unique(np.concatenate([s, d]), return_counts=True)
    deg = dict(zip(ids.tolist(), cnt.tolist()))
    du = np.array([deg[a] for a in rs.tolist()])
    dv = np.array([deg[b] for b in rd.tolist()])
    slen, llen = np.minimum(du, dv), np.maximum(du, dv)
    workgroup = int(np.sum((slen > WAVE_ROW) & (llen >= LDS_ROW)))
    wave = int(np.sum(slen > SHORT_ROW)) - workgroup
    return wave, workgroup, int(slen.sum())


@pytest.mark.parametrize("several", [1, 5], ids=["one_per_bin", "five_per_bin"])
@pytest.mark.parametrize("D", [LDS_ROW - 1, LDS_ROW])
@pytest.mark.parametrize("c", [SHORT_ROW, SHORT_ROW + 1, WAVE_ROW, WAVE_ROW + 1])
def test_dying_edges_in_every_bin(gs, variant, c, D, several):
    """Dying edges with shorter rows of 1, SHORT_ROW | SHORT_ROW + 1 | WAVE_ROW | WAVE_ROW + 1
    against longer rows of the same length and of LDS_ROW - 1 | LDS_ROW: a lane group, a wave or
    a workgroup each, as a fold would bin them. The removal's own lists and steps equal the host
    model on the degrees before the removal; the fold's diagnostics stay what they were."""
    hub, mids, leaves, s, d = _hub_and_clique(c, D)
    k = several
    rs = np.concatenate([np.full(k, hub, np.int64), mids[:k], mids[1:1 + k]])
    rd = np.concatenate([leaves[7:7 + k], np.full(k, hub, np.int64), mids[k + 1:2 * k + 1]])
    assert len(set(_Model._pairs(rs, rd))) == 3 * k
    wave, workgroup, steps = _removal_model(s, d, rs, rd)
    big = c > WAVE_ROW and D >= LDS_ROW
    assert (wave, workgroup) == ((0, 0) if c <= SHORT_ROW else (k, k) if big else (2 * k, 0))
    assert steps == k + 2 * k * c
    with gs.SlidingTriangles(edge_hint=64) as T:
        T.fold(s, d)
        before, bins, t0 = T.stats(), T.bins(), T.count()[0]
        T.remove(rs, rd)
        ks, kd = _without(s, d, rs, rd)
        ids, t, total, edges = _check(T, ks, kd, absent=leaves[7:7 + k])
        st = T.remove_stats()
        assert (st["edges_removed"], st["vertices_vanished"]) == (3 * k, k)
        assert st["triangles_destroyed"] == t0 - total and t0 > total
        assert (st["wave_list"], st["workgroup_list"]) == ((wave, workgroup) if variant == 0 else (0, 0))
        assert st["steps"] == steps
        after = T.stats()
        assert (after["steps"], after["hot_row"]) == (before["steps"], before["hot_row"]) and T.bins() == bins


# ------------------------------------------------------------------ 6. equivalence on a graph with hubs
def _rmat(scale, n, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros(n, np.int64)
    d = np.zeros(n, np.int64)
    for _ in range(scale):
        q = rng.choice(4, size=n, p=[0.57, 0.19, 0.19, 0.05])
        s = (s << 1) | (q >> 1)
        d = (d << 1) | (q & 1)
    scr = lambda x: (x.astype(np.uint64) * MULT + np.uint64(12345)).view(np.int64)  # 64-bit ids
    return scr(s), scr(d)


_STREAM = {}


def _xyz():
    """X: RMAT scale 12, 2^15 edges, scrambled ids. Y: a seeded 30 % sample of X and a tenth as
    many absent pairs. Z: half of Y's present pairs and fresh pairs."""
    if not _STREAM:
        xs, xd = _rmat(12, 1 << 15, 0xE1)
        rng = np.random.default_rng(0xE2)
        take = rng.random(len(xs)) < 0.3
        fs, fd = _rmat(12, len(xs) // 10, 0xE3)  # mostly absent from X
        ys, yd = np.concatenate([xs[take], fd]), np.concatenate([xd[take], fs])
        p = rng.permutation(len(ys))
        ys, yd = ys[p], yd[p]
        zs, zd = _rmat(12, 4000, 0xE4)
        zs, zd = np.concatenate([ys[::2], zs]), np.concatenate([yd[::2], zd])
        _STREAM["xyz"] = (xs, xd), (ys, yd), (zs, zd)
    return _STREAM["xyz"]


def _pieces(a, b, k):
    cut = np.linspace(0, len(a), k + 1).astype(int)
    return [(a[i:j], b[i:j]) for i, j in zip(cut[:-1], cut[1:])]


@pytest.mark.parametrize("rk", [1, 4])
@pytest.mark.parametrize("fk", [1, 3, 16])
def test_fold_remove_fold_on_rmat(gs, variant, fk, rk):
    (xs, xd), (ys, yd), (zs, zd) = _xyz()
    M = _Model()
    with gs.SlidingTriangles(edge_hint=1 << 10) as T:
        for ps, pd in _pieces(xs, xd, fk):
            T.fold(ps, pd)
            M.fold(ps, pd)
            _check(T, *M.edges())
        e0 = T.count()[1]
        for ps, pd in _pieces(ys, yd, rk):
            T.remove(ps, pd)
            M.remove(ps, pd)
            _check(T, *M.edges(), absent=np.concatenate([xs[:2000], ys[:2000]]))
        assert 0.4 * e0 < T.count()[1] < 0.8 * e0  # a repeated pair is sampled more often than once
        T.fold(zs, zd)
        M.fold(zs, zd)
        _check(T, *M.edges())


def test_device_entry_points_with_a_stride(gs, variant):
    """fold_device / remove_device, stride 2, interleaved: the odd elements are poison."""
    import torch
    (xs, xd), (ys, yd), (zs, zd) = _xyz()
    M = _Model()

    def strided(a):
        out = np.full(2 * len(a), 0x0BAD, np.int64)
        out[::2] = a
        return out

    with gs.SlidingTriangles(edge_hint=1 << 10) as T:
        steps = [("fold", xs[:20000], xd[:20000]), ("remove", ys[:6000], yd[:6000]), ("fold", xs[20000:], xd[20000:]),
                 ("remove", ys[6000:], yd[6000:]), ("fold", zs, zd), ("remove", zs[:0], zd[:0])]
        for what, a, b in steps:
            ta, tb = _dev(T, strided(a)), _dev(T, strided(b))
            torch.cuda.synchronize()
            getattr(T, what + "_device")(ta, tb, n=len(a), stride=2)
            getattr(M, what)(a, b)
            _check(T, *M.edges())


# ------------------------------------------------------------------ 7. expiry
def _panes(n, seed, empty=()):
    """n panes over 40 vertices that share many edges; the panes in `empty` hold nothing."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = 0 if k in empty else int(rng.integers(20, 60))
        s, d = rng.integers(0, 40, m), rng.integers(0, 40, m)
        out.append(((s.astype(np.uint64) * MULT).view(np.int64), (d.astype(np.uint64) * MULT).view(np.int64)))
    return out


def test_slide_by_one_pane_is_a_tumbling_window(gs, variant):
    """(With refresh: an edge that two consecutive panes share belongs to the later one too.
    Without it the edge keeps the earlier pane's stamp and leaves with it, as the next test
    models.)"""
    with gs.SlidingTriangles(edge_hint=64, refresh=True) as S, gs.SlidingTriangles(edge_hint=64) as W:
        for s, d in _panes(8, 0x51, empty=(3,)):
            assert S.slide(s, d, 1) == W.window(s, d)
            _check(S, s, d)


@pytest.mark.parametrize("W", [1, 2, 5])
@pytest.mark.parametrize("refresh", [True, False], ids=["refresh", "first_added"])
def test_sliding_windows_over_twelve_panes(gs, variant, refresh, W):
    """With refresh the graph is the union of the last W panes; without, the pairs first added in
    the last W folds (a pair that is still held keeps its old stamp). Panes 4 and 9 are empty:
    they age the others all the same."""
    panes = _panes(12, 0x52, empty=(4, 9))
    M = _Model(refresh=refresh)
    every = np.unique(np.concatenate([p[0] for p in panes] + [p[1] for p in panes]))
    differs = False
    with gs.SlidingTriangles(edge_hint=64, refresh=refresh) as T:
        for k, (s, d) in enumerate(panes):
            got = T.slide(s, d, W)
            M.fold(s, d)
            M.expire(W)
            ids, t, total, edges = _check(T, *M.edges(), absent=every)
            assert got == total
            if refresh:
                us = np.concatenate([p[0] for p in panes[max(0, k + 1 - W):k + 1]])
                ud = np.concatenate([p[1] for p in panes[max(0, k + 1 - W):k + 1]])
                assert _truth(us, ud)[3] == edges  # the model IS the union of the last W panes
            else:
                us = np.concatenate([p[0] for p in panes[max(0, k + 1 - W):k + 1]])
                ud = np.concatenate([p[1] for p in panes[max(0, k + 1 - W):k + 1]])
                differs = differs or _truth(us, ud)[3] != edges
    assert refresh or W == 1 or differs  # the two stamps are told apart by this stream


def test_expire_beyond_the_folds_made_removes_nothing(gs):
    s, d = _clique([1, 2, 3, 4])
    with gs.SlidingTriangles(edge_hint=16) as T:
        assert gs.lib().gs_triangle_expire(T.handle, 0) == gs.GS_ERR_INVALID
        T.expire(1)  # no fold yet
        T.fold(s[:3], d[:3])
        T.fold(s[3:], d[3:])
        T.fold(s[:0], d[:0])  # fold 3, of nothing
        for folds in (1 << 40, 4, 3):
            T.expire(folds)
            assert T.remove_stats()["edges_removed"] == 0
            _check(T, s, d)
        T.expire(2)  # fold 1 is older than the last two
        assert T.remove_stats()["edges_removed"] == 3
        _check(T, s[3:], d[3:])
        T.expire(1)
        assert T.count() == (0, 0, 0)


# ------------------------------------------------------------------ 8. the fold number's wrap
@pytest.mark.parametrize("refresh", [True, False], ids=["refresh", "first_added"])
def test_slide_across_the_wrap_of_the_fold_number(gs, refresh):
    panes = _panes(6, 0x53)
    M = _Model(refresh=refresh)
    with gs.SlidingTriangles(edge_hint=64, refresh=refresh) as T:
        assert gs.lib().gs_testing_triangle_set_fold(T.handle, (1 << 32) - 4) == gs.GS_OK  # folds ..FD, FE, FF, wrap
        for s, d in panes:
            got = T.slide(s, d, 3)
            M.fold(s, d)
            M.expire(3)
            assert got == _check(T, *M.edges())[2]
        assert gs.lib().gs_testing_triangle_set_fold(T.handle, 5) == gs.GS_ERR_INVALID  # it holds edges


# ------------------------------------------------------------------ 9. the table does not grow under a window
def test_table_stays_its_size_under_a_sliding_window(gs):
    M = _Model()
    slots = {}
    with gs.SlidingTriangles(edge_hint=8) as T:
        for k in range(1, 65):
            base = 1000 * k
            s, d = _clique([base + j for j in range(9)])  # 36 edges on 9 ids that never recur
            T.slide(s, d, 2)
            M.fold(s, d)
            M.expire(2)
            _check(T, *M.edges(), absent=[base - 1000 * 2 + j for j in range(9)])
            slots[k] = T.remove_stats()["table_slots"]
            assert T.count()[2] == (9 if k == 1 else 18)
    assert slots[64] == slots[4]
