"""GPU: the triangle streams (gsamd.TriangleStream, the gs_tristream_* calls) against a Python
model of the sequential definition (include/gs_summary.h: rules 1 - 6) and against the pins of
tests/golden/tristream_pins.json. Every output is an integer: comparisons are exact."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
SENTINEL = 0x5A5A5A5B


def _pins():
    with open(os.path.join(GOLD, "tristream_pins.json")) as f:
        return json.load(f)


class Model:
    """The sequential definition, one arrival after the other."""

    def __init__(self, repeats="count"):
        self.repeats = repeats
        self.first = {}
        self.nb = {}
        self.t = {}
        self.total = 0
        self.arrivals = 0
        self.seen = {}  # id -> rank: the order of first appearance, loops included

    def fold(self, src, dst):
        rows, recs = [], []
        for a in range(len(src)):
            self.arrivals += 1
            t = self.arrivals
            s, d = int(src[a]), int(dst[a])
            for x in (s, d):
                self.seen.setdefault(x, len(self.seen))
            if s == d:
                rows.append((0, self.total))
                continue
            u, v = min(s, d), max(s, d)
            was = (u, v) in self.first
            if not was:
                self.first[(u, v)] = t
                self.nb.setdefault(u, {})[v] = t
                self.nb.setdefault(v, {})[u] = t
            C = []
            if not (self.repeats == "ignore" and was):
                nu, nv = self.nb[u], self.nb[v]
                small, big = (nu, nv) if len(nu) <= len(nv) else (nv, nu)
                C = sorted(w for w, f in small.items() if f < t and big.get(w, t) < t)
            c = len(C)
            for w in C:
                self.t[w] = self.t.get(w, 0) + 1
                recs.append((a, w, self.t[w]))
            if c:
                for x in (u, v):
                    self.t[x] = self.t.get(x, 0) + c
                    recs.append((a, x, self.t[x]))
                self.total += c
            rows.append((c, self.total))
        return rows, recs

    def counts(self):
        return sorted((v, c) for v, c in self.t.items() if c > 0)

    def vertices(self):
        return len(self.nb)

    def crossed(self, recs, tile):
        """Tiles of the record scan (records sorted stably by rank) that begin inside a segment."""
        order = sorted(range(len(recs)), key=lambda r: self.seen[recs[r][1]])
        return sum(1 for j in range(tile, len(recs), tile) if recs[order[j]][1] == recs[order[j - 1]][1])


def _got(S):
    c, t = S.rows()
    a, v, k = S.records()
    return list(zip(c.tolist(), t.tolist())), list(zip(a.tolist(), v.tolist(), k.tolist()))


def _check_state(S, M):
    v, c = S.local_counts()
    assert list(zip(v.tolist(), c.tolist())) == M.counts()
    assert S.count() == {"triangles": M.total, "edges": len(M.first), "vertices": M.vertices(), "arrivals": M.arrivals}


def _fold_both(S, M, src, dst):
    """One fold through the handle and the model; rows, records and state compared."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    before = len(M.first)
    S.fold(src, dst)
    rows, recs = M.fold(src, dst)
    got_rows, got_recs = _got(S)
    assert got_rows == rows
    assert got_recs == recs
    s = S.size()
    assert (s["arrivals"], s["records"], s["new_pairs"], s["total"]) == (len(rows), len(recs), len(M.first) - before,
                                                                         M.arrivals)
    _check_state(S, M)
    return rows, recs


def _stream(rng, n, vertices, loops=0.05):
    s = rng.integers(0, vertices, n).astype(np.int64)
    d = rng.integers(0, vertices, n).astype(np.int64)
    keep = (s != d) | (rng.random(n) < loops)
    d = np.where(keep, d, (d + 1) % vertices)
    return s, d


def _folds(S, M, src, dst, sizes):
    """The stream in consecutive folds of the given sizes (cycled); the concatenated rows and
    records with stream-wide arrival indices."""
    rows, recs, at = [], [], 0
    for size in itertools.cycle(sizes):
        if at >= len(src):
            break
        r, c = _fold_both(S, M, src[at:at + size], dst[at:at + size])
        rows += r
        recs += [(a + at, v, k) for a, v, k in c]
        at += size
    return rows, recs


# ---------------------------------------------------------------- pins and the single triangle
def test_pinned_intersections_and_the_worked_example(gs):
    pins = _pins()
    for case in pins["test_intersection"]["cases"]:
        e = np.array(case["as_stream"], np.int64)
        with gs.TriangleStream(edge_hint=16) as S:
            rows, recs = _fold_both(S, Model(), e[:, 0], e[:, 1])
        assert [[v, c] for _, v, c in recs] == case["stream_records"]
        assert all(a == len(e) - 1 for a, _, _ in recs) and rows[-1] == (2, case["stream_total"])
        assert sorted([[v, c] for _, v, c in recs] + [[-1, rows[-1][1]]]) == sorted(case["expected_tuples"])
    e = np.array(pins["builtin_stream"]["edges"], np.int64)
    d = pins["derived"]
    for sizes in ((9,), (1,), (4, 5), (8, 1)):
        with gs.TriangleStream() as S:
            rows, recs = _folds(S, Model(), e[:, 0], e[:, 1], sizes)
        assert [list(r) for r in recs] == d["records"]
        assert [r[0] for r in rows] == d["closed"] and [r[1] for r in rows] == d["totals"]


@pytest.mark.parametrize("sizes", [(1,), (2, 1), (3,)], ids=["three-folds", "two-and-one", "one-fold"])
def test_one_triangle_in_every_order_and_orientation(gs, sizes):
    edges = [(10, 20), (20, 30), (10, 30)]
    for order in itertools.permutations(edges):
        for flip in (False, True):
            src = [b if flip else a for a, b in order]
            dst = [a if flip else b for a, b in order]
            with gs.TriangleStream(edge_hint=4) as S:
                rows, recs = _folds(S, Model(), np.array(src), np.array(dst), sizes)
            assert rows == [(0, 0), (0, 0), (1, 1)]
            u, v = sorted(order[2])
            w = ({10, 20, 30} - {u, v}).pop()
            assert recs == [(2, w, 1), (2, u, 1), (2, v, 1)]


def test_the_stamp_filter_inside_one_fold(gs):
    # u-w, u-v, v-w in ONE fold: the merged adjacency holds {v, w} when arrival 2 is intersected
    u, v, w = 5, 7, 9
    with gs.TriangleStream() as S:
        rows, recs = _fold_both(S, Model(), [u, u, v], [w, v, w])
    assert rows == [(0, 0), (0, 0), (1, 1)]
    assert recs == [(2, u, 1), (2, v, 1), (2, w, 1)]  # arrival 3 closes with w' = u; then min, max of (v, w)


# ---------------------------------------------------------------- repeats
def test_repeats_count_again_or_not_at_all(gs):
    src, dst = [1, 2, 1, 1, 3, 2, 2], [2, 3, 3, 3, 1, 1, 1]
    with gs.TriangleStream("count") as S:
        rows, recs = _fold_both(S, Model("count"), src, dst)
    assert [r[0] for r in rows] == [0, 0, 1, 1, 1, 1, 1] and rows[-1][1] == 5 and len(recs) == 15
    with gs.TriangleStream("ignore") as S:
        rows, recs = _fold_both(S, Model("ignore"), src, dst)
    assert [r[0] for r in rows] == [0, 0, 1, 0, 0, 0, 0] and rows[-1][1] == 1 and len(recs) == 3
    # the same, the repeats in folds of their own
    for mode in ("count", "ignore"):
        with gs.TriangleStream(mode) as S:
            M = Model(mode)
            _folds(S, M, np.array(src), np.array(dst), (3, 1, 2, 1))
            assert M.total == (5 if mode == "count" else 1)


def test_a_repeat_before_the_closing_edge_never_counts_twice(gs):
    # 1-2 twice, 2-3 twice, then 1-3: one triangle, whatever the mode; w = 2 is one neighbour
    for mode in ("count", "ignore"):
        with gs.TriangleStream(mode) as S:
            rows, recs = _fold_both(S, Model(mode), [1, 2, 2, 3, 1], [2, 1, 3, 2, 3])
        assert [r[0] for r in rows] == [0, 0, 0, 0, 1] and recs == [(4, 2, 1), (4, 1, 1), (4, 3, 1)]


def test_a_repeat_inside_the_fold_that_adds_the_pair(gs):
    # 1-2, 2-3 first; then ONE fold 1-3, 3-1, 1-3: the pair is new in this fold, its repeats follow
    for mode, closed in (("count", [1, 1, 1]), ("ignore", [1, 0, 0])):
        with gs.TriangleStream(mode) as S:
            M = Model(mode)
            _fold_both(S, M, [1, 2], [2, 3])
            rows, _ = _fold_both(S, M, [1, 3, 1], [3, 1, 3])
            assert [r[0] for r in rows] == closed and S.size()["new_pairs"] == 1


# ---------------------------------------------------------------- ordered write
# The closing arrival walks a row of d + 1 entries (the hub-hub entry is in it). A lane group walks
# in chunks of TRISTREAM_LANES = 8 (7 .. 9, 15 .. 17), a row of more than TRISTREAM_SHORT_ROW = 32
# entries takes a wave (30 .. 33) that walks in chunks of 64 (62 .. 66, 127 .. 129).
HUB_D = (1, 7, 8, 9, 15, 16, 17, 30, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1025)


def test_the_hub_sizes_sit_on_the_kernels_thresholds(gs):
    L, S = gs.TRISTREAM_LANES, gs.TRISTREAM_SHORT_ROW
    for row in (L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, S - 1, S, S + 1, S + 2, 63, 64, 65, 127, 128, 129):
        assert row - 1 in HUB_D or row in HUB_D, row
    for d in (S - 2, S - 1, S, S + 1, 63, 64, 65):
        assert d in HUB_D, d


@pytest.mark.parametrize("d", HUB_D)
@pytest.mark.parametrize("longer", ["first", "second"])
def test_two_hubs_emit_their_common_neighbours_in_ascending_order(gs, d, longer):
    h1, h2 = 100000, 100001
    extra = np.arange(200000, 200000 + 70, dtype=np.int64)  # one hub's row is longer by these
    w = np.arange(1, d + 1, dtype=np.int64)[::-1].copy()  # arrival order descending: the records ascend
    src = np.concatenate([np.full(d, h1), np.full(d, h2), np.full(len(extra), h1 if longer == "first" else h2), [h1]])
    dst = np.concatenate([w, w, extra, [h2]])
    with gs.TriangleStream(edge_hint=16) as S:
        rows, recs = _fold_both(S, Model(), src, dst)
        assert S.stats()["longest_row"] == d + 71
    assert rows[-1] == (d, d)
    assert [v for _, v, _ in recs] == list(range(1, d + 1)) + [h1, h2]
    assert [c for _, _, c in recs] == [1] * d + [d, d]


# ---------------------------------------------------------------- segmented scan over tiles
def _scan_case(tile, which):
    """m and the number of 4-record gadgets with R = 3 (m - 1) + 4 k."""
    want = {"T-1": tile - 1, "T": tile, "T+1": tile + 1, "3T+5": 3 * tile + 5}[which]
    for k in range(3):
        if (want - 4 * k) % 3 == 0:
            return want, (want - 4 * k) // 3 + 1, k
    raise AssertionError(which)


@pytest.mark.parametrize("which", ["T-1", "T", "T+1", "3T+5"])
def test_a_segment_crosses_tiles_and_the_next_fold_starts_from_the_counters(gs, which):
    T = gs.TRISTREAM_TILE
    R, m, k = _scan_case(T, which)
    w = 5000000
    ids = np.arange(1, m + 1, dtype=np.int64)
    gadget = [(9000000 + 10 * g) for g in range(k)]  # a, b = a + 1, x = a + 2, y = a + 3
    with gs.TriangleStream(edge_hint=16) as S:
        M = Model()
        # loops give every path vertex a rank before w: w's segment ends the sorted records
        _fold_both(S, M, ids, ids)
        src = [np.full(m, w), ids[:-1]]
        dst = [ids, ids[1:]]
        for a in gadget:
            src.append(np.array([a, a, a + 1, a + 1, a]))
            dst.append(np.array([a + 2, a + 3, a + 2, a + 3, a + 1]))
        rows, recs = _fold_both(S, M, np.concatenate(src), np.concatenate(dst))
        assert len(recs) == R and sum(1 for _, v, _ in recs if v == w) == m - 1
        st = S.stats()
        assert st["tiles"] == (R + T - 1) // T
        assert st["crossed"] == M.crossed(recs, T)
        if which in ("T+1", "3T+5"):
            assert st["crossed"] >= 1
        # the same vertices again: every count continues from the stored counter
        rows2, recs2 = _fold_both(S, M, ids[:-2], ids[2:])
        assert all(c == 2 for c, _ in rows2) and recs2[0] == (0, 2, 3)
        assert [k for _, v, k in recs2 if v == w] == list(range(m, 2 * m - 2))


# ---------------------------------------------------------------- ids
def test_extreme_ids_and_signed_order(gs):
    lo, hi = I64_MIN, I64_MAX
    with gs.TriangleStream() as S:
        M = Model()
        rows, recs = _fold_both(S, M, [lo, lo, hi, hi, lo, lo, hi, lo], [5, -1, 5, -1, hi, 0, 0, hi])
        assert [v for a, v, _ in recs if a == 4] == [-1, 5, lo, hi]
        assert [v for a, v, _ in recs if a == 7] == [-1, 0, 5, lo, hi]
        v, c = S.local_counts()
        assert v.tolist() == [lo, -1, 0, 5, hi]
        # -1 closing its own triangle: a vertex like any other
        _fold_both(S, M, [-1], [5])
        _fold_both(S, M, [lo, hi, lo], [lo, hi, hi])  # loops of the extremes, a repeat


# ---------------------------------------------------------------- cut invariance
def _dense(rng):
    """600 arrivals over 64 vertices: every 37th a loop, two in five of the later ones a repeat of
    an earlier arrival, half of those turned round."""
    s, d = _stream(rng, 600, 64, loops=0.0)
    for i in range(300, 600):
        if rng.random() < 0.4:
            j = int(rng.integers(0, i))
            s[i], d[i] = (d[j], s[j]) if rng.random() < 0.5 else (s[j], d[j])
    d[::37] = s[::37]
    return s, d


@pytest.fixture(scope="module")
def dense_model():
    src, dst = _dense(np.random.default_rng(41))
    out = {}
    for mode in ("count", "ignore"):
        M = Model(mode)
        out[mode] = M.fold(src, dst) + (M,)
    return src, dst, out


@pytest.mark.parametrize("sizes", [(600,), (1,), (2,), (63,), (64,), (65,), (257,), "seeded"],
                         ids=["whole", "1", "2", "63", "64", "65", "257", "three-way"])
@pytest.mark.parametrize("mode", ["count", "ignore"])
def test_rows_and_records_do_not_depend_on_the_cut(gs, dense_model, mode, sizes):
    src, dst, model = dense_model
    rows, recs, whole = model[mode]
    loops = sum(1 for s, d in zip(src, dst) if s == d)
    assert loops > 10 and len(whole.first) + loops < 600 - 50  # loops, repeats
    if sizes == "seeded":
        a, b = sorted(np.random.default_rng(7).integers(1, 599, 2).tolist())
        sizes = (a, b - a, 600 - b)
    with gs.TriangleStream(mode, edge_hint=16) as S:
        M = Model(mode)
        got_rows, got_recs = _folds(S, M, src, dst, sizes)
        assert got_rows == rows and got_recs == recs
        assert M.counts() == whole.counts()


# ---------------------------------------------------------------- the existing handle
def test_ignore_mode_ends_where_the_triangle_summary_ends(gs):
    rng = np.random.default_rng(3)
    src, dst = _stream(rng, 3000, 200, loops=0.3)
    with gs.Triangles(edge_hint=16) as Tr:
        Tr.fold(src, dst)
        t, e, nv = Tr.count()
        tv, tc = Tr.local_counts(nonzero_only=True)
    assert t > 0
    with gs.TriangleStream("ignore", edge_hint=16) as S:
        for at in range(0, 3000, 700):
            S.fold(src[at:at + 700], dst[at:at + 700])
        c = S.count()
        v, k = S.local_counts()
    assert (c["triangles"], c["edges"], c["vertices"]) == (t, e, nv)
    assert np.array_equal(v, tv) and np.array_equal(k, tc)
    # count mode agrees on the de-duplicated stream
    seen, keep = set(), []
    for i, (a, b) in enumerate(zip(src.tolist(), dst.tolist())):
        key = (min(a, b), max(a, b))
        if a != b and key not in seen:
            seen.add(key)
            keep.append(i)
    with gs.TriangleStream("count", edge_hint=16) as S:
        S.fold(src[keep], dst[keep])
        assert S.count()["triangles"] == t
        v, k = S.local_counts()
    assert np.array_equal(v, tv) and np.array_equal(k, tc)


# ---------------------------------------------------------------- growth, reset, device forms
def test_growth_from_a_small_hint(gs):
    rng = np.random.default_rng(5)
    src, dst = _stream(rng, 4000, 300)
    with gs.TriangleStream(edge_hint=16) as S:
        M = Model()
        for at in range(0, 4000, 800):
            _fold_both(S, M, src[at:at + 800], dst[at:at + 800])
        assert len(M.first) > 2000


def test_reset_and_empty_fold(gs):
    with gs.TriangleStream() as S:
        S.fold([], [])
        assert S.size() == {"arrivals": 0, "records": 0, "new_pairs": 0, "total": 0}
        assert _got(S) == ([], []) and len(S.local_counts()[0]) == 0
        M = Model()
        _fold_both(S, M, [1, 2, 3, 4, 4], [2, 3, 1, 4, 1])
        S.fold([], [])
        assert _got(S) == ([], [])  # the last fold had no rows
        _check_state(S, M)
        _fold_both(S, M, [7, 7, 7], [7, 7, 7])  # loops only
        S.reset()
        assert S.count() == {"triangles": 0, "edges": 0, "vertices": 0, "arrivals": 0}
        assert len(S.local_counts()[0]) == 0
        _fold_both(S, Model(), [1, 2, 3, 4, 4], [2, 3, 1, 4, 1])  # a reused handle equals a fresh one


def test_device_folds_and_reads_with_sentinels(gs):
    import torch
    rng = np.random.default_rng(9)
    n = 700
    src, dst = _stream(rng, n, 40)
    dev = torch.device("cuda", 0)
    with gs.TriangleStream(edge_hint=16) as S:
        M = Model()
        rows, recs = M.fold(src, dst)
        # strided device arrays: element i at index 2 i
        ts = torch.from_numpy(np.repeat(src, 2)).to(dev)
        td = torch.from_numpy(np.repeat(dst, 2)).to(dev)
        S.fold_device(ts, td, n=n, stride=2, after="torch")
        S.sync()
        assert _got(S) == (rows, recs)
        m, r = len(rows), len(recs)
        tc = torch.full((m + 1,), SENTINEL, dtype=torch.int32, device=dev)
        tt = torch.full((m + 1,), SENTINEL, dtype=torch.int64, device=dev)
        ra = torch.full((r + 1,), SENTINEL, dtype=torch.int32, device=dev)
        rv, rk = (torch.full((r + 1,), SENTINEL, dtype=torch.int64, device=dev) for _ in range(2))
        S.wait_stream("torch")
        assert S.rows_device(tc, tt) == m and S.records_device(ra, rv, rk) == r
        S.sync()
        assert list(zip(tc[:m].tolist(), tt[:m].tolist())) == rows
        assert list(zip(ra[:r].tolist(), rv[:r].tolist(), rk[:r].tolist())) == recs
        k = len(M.counts())
        cv, cc = (torch.full((k + 1,), SENTINEL, dtype=torch.int64, device=dev) for _ in range(2))
        S.wait_stream("torch")
        assert S.local_counts_device(cv, cc) == k
        S.sync()
        assert list(zip(cv[:k].tolist(), cc[:k].tolist())) == M.counts()
        for t in (tc, tt, ra, rv, rk, cv, cc):
            assert int(t[-1]) == SENTINEL
        # too small arrays: the count, nothing written
        small = torch.full((3,), SENTINEL, dtype=torch.int64, device=dev)
        for call in (lambda: S.rows_device(None, small), lambda: S.records_device(None, small, None),
                     lambda: S.local_counts_device(small, None)):
            with pytest.raises(gs.GSError) as e:
                call()
            assert e.value.code == gs.GS_ERR_TRUNCATED
        S.sync()
        assert small.tolist() == [SENTINEL] * 3
        # the host forms: the count, nothing written
        got = ctypes.c_size_t(0)
        buf = np.full(3, SENTINEL, np.int64)
        L = gs.lib()
        assert L.gs_tristream_rows(S._h, None, buf.ctypes.data, 3, ctypes.byref(got)) == gs.GS_ERR_TRUNCATED
        assert got.value == m
        assert L.gs_tristream_records(S._h, None, buf.ctypes.data, None, 3, ctypes.byref(got)) == gs.GS_ERR_TRUNCATED
        assert got.value == r
        assert L.gs_tristream_counts(S._h, buf.ctypes.data, None, 3, ctypes.byref(got)) == gs.GS_ERR_TRUNCATED
        assert got.value == k and buf.tolist() == [SENTINEL] * 3
        with pytest.raises(gs.GSError) as e:
            S.fold_device(ts, td, n=n, stride=0)
        assert e.value.code == gs.GS_ERR_INVALID


# ---------------------------------------------------------------- the limits
def test_the_arrival_limit_is_checked_before_any_work(gs):
    with gs.TriangleStream() as S:
        M = Model()
        _fold_both(S, M, [1, 2, 3], [2, 3, 1])
        before = (_got(S), S.count(), S.size())
        a = np.zeros(4, np.int64)
        L = gs.lib()
        # 3 + (2^31 - 3) arrivals: one too many; the arrays are never read
        rc = L.gs_tristream_fold(S._h, a.ctypes.data, a.ctypes.data, gs.TRISTREAM_MAX_TOTAL - 2)
        assert rc == gs.GS_ERR_CAPACITY and b"2^31 - 1" in L.gs_last_error()
        rc = L.gs_tristream_fold_device(S._h, a.ctypes.data, a.ctypes.data, gs.TRISTREAM_MAX_TOTAL + 1, 1)
        assert rc == gs.GS_ERR_CAPACITY
        assert (_got(S), S.count(), S.size()) == before
        _fold_both(S, M, [1, 4, 4], [4, 2, 3])


def test_a_fold_past_the_record_limit_changes_nothing(gs):
    rng = np.random.default_rng(11)
    src, dst = _stream(rng, 300, 24)
    whole = Model()
    whole.fold(src[:100], dst[:100])
    _, a = whole.fold(src[100:200], dst[100:200])
    _, b = whole.fold(src[200:], dst[200:])
    limit = max(len(a), len(b))  # each piece fits, the two in one fold do not
    assert 0 < min(len(a), len(b))
    with gs.TriangleStream(edge_hint=16) as S:
        M = Model()
        _fold_both(S, M, src[:100], dst[:100])
        before = (_got(S), S.count(), [x.tolist() for x in S.local_counts()], S.size())
        S.tune(max_records=limit)
        with pytest.raises(gs.GSError) as e:
            S.fold(src[100:], dst[100:])
        assert e.value.code == gs.GS_ERR_CAPACITY and "records" in str(e.value)
        assert (_got(S), S.count(), [x.tolist() for x in S.local_counts()], S.size()) == before
        # the same stream in two pieces
        _fold_both(S, M, src[100:200], dst[100:200])
        _fold_both(S, M, src[200:], dst[200:])
        assert M.counts() == whole.counts() and M.total == whole.total
        with pytest.raises(gs.GSError):
            S.tune(max_records=gs.TRISTREAM_MAX_RECORDS + 1)
        S.tune(max_records=0)  # the product value again
        _fold_both(S, M, src, dst)
