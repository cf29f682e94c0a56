"""GPU: the degree streams (gsamd.DegreeStream, the gs_degstream_* calls) against a Python model
of the sequential rule (include/gs_summary.h: rows old -> new = max(old + c, 0), records, counts)
and against the reference's pinned outputs (tests/golden/degree_pins.json: every emitted value,
in order). Every output is an integer: comparisons are exact."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
SENTINEL = 0x5A5A5A5B
DIRS = ("all", "in", "out")
FAR = 1 << 40  # ids of endpoints that direction "out" does not collect


def _pins():
    with open(os.path.join(GOLD, "degree_pins.json")) as f:
        return json.load(f)


def _sizes(gs):
    T = gs.DEGSTREAM_TILE
    return (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5)


class Model:
    """The sequential definition, one occurrence after the other."""

    def __init__(self, direction):
        self.direction = direction
        self.deg = {}
        self.cnt = {}
        self.total = 0

    def fold(self, src, dst, dele=None):
        rows, recs = [], []
        o = 0
        for i in range(len(src)):
            c = -1 if dele is not None and (int(dele[i]) & 1) else 1
            ends = {"all": (src[i], dst[i]), "out": (src[i],), "in": (dst[i],)}[self.direction]
            for v in ends:
                v = int(v)
                old = self.deg.get(v, 0)
                new = max(old + c, 0)
                self.deg[v] = new
                rows.append((v, old, new))
                if old > 0:
                    rec = ([(new, 1)] if new > 0 else []) + [(old, -1)]
                else:
                    rec = [(1, 1)] if c > 0 else []
                for d, delta in rec:
                    self.cnt[d] = self.cnt.get(d, 0) + delta
                    assert self.cnt[d] >= 0
                    recs.append((o, d, self.cnt[d]))
                o += 1
        self.total += o
        return rows, recs

    def degrees(self):
        return sorted((v, d) for v, d in self.deg.items() if d > 0)

    def distribution(self):
        return sorted((d, c) for d, c in self.cnt.items() if c > 0)


def _got(D):
    v, o, w = D.rows()
    ro, rd, rc = D.records()
    return (list(zip(v.tolist(), o.tolist(), w.tolist())), list(zip(ro.tolist(), rd.tolist(), rc.tolist())))


def _check_state(D, M):
    v, d = D.degrees()
    assert list(zip(v.tolist(), d.tolist())) == M.degrees()
    g, c = D.distribution()
    assert list(zip(g.tolist(), c.tolist())) == M.distribution()
    assert D.size()["total"] == M.total
    assert D.size()["max_degree"] >= max([x for _, x in M.degrees()] + [0])


def _fold_both(D, M, src, dst, dele=None):
    """One fold through the handle and the model; rows, records and state compared."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    dele = None if dele is None else np.asarray(dele, np.uint8)
    D.fold(src, dst, dele)
    rows, recs = M.fold(src, dst, dele)
    got_rows, got_recs = _got(D)
    assert got_rows == rows
    assert got_recs == recs
    s = D.size()
    assert (s["occurrences"], s["records"]) == (len(rows), len(recs))
    _check_state(D, M)
    return rows, recs


def _out_edges(vertices, signs):
    """Occurrence lists as edges of direction "out": one occurrence per edge."""
    v = np.asarray(vertices, np.int64)
    dele = (np.asarray(signs) < 0).astype(np.uint8)
    return v, v + FAR, dele


# ---------------------------------------------------------------- the pins
@pytest.mark.parametrize("name,direction", [("get_degrees", "all"), ("get_in_degrees", "in"), ("get_out_degrees", "out")])
def test_pinned_running_degrees(gs, name, direction):
    pins = _pins()
    e = np.array(pins["sample_edges"]["edges"], np.int64)
    assert pins[name]["direction"] == direction
    with gs.DegreeStream(direction, vertex_hint=16) as D:
        D.fold(e[:, 0], e[:, 1])
        v, old, new = D.rows()
        assert sorted("%d,%d" % (a, b) for a, b in zip(v.tolist(), new.tolist())) == sorted(pins[name]["lines"])
        assert np.array_equal(new, old + 1)  # no deletions: what DegreeMapFunction emits


@pytest.mark.parametrize("data,result", [("degrees_data", "degrees_result"), ("degrees_data_zero", "degrees_result_zero")])
@pytest.mark.parametrize("cut", [None, 1, 3, 5])
def test_pinned_distribution_records_in_order(gs, data, result, cut):
    pins = _pins()
    ev = [ln.split() for ln in pins[data]["text"].split("\n")]
    src = np.array([int(x[0]) for x in ev], np.int64)
    dst = np.array([int(x[1]) for x in ev], np.int64)
    dele = np.array([1 if x[2] == "-" else 0 for x in ev], np.uint8)
    got = []
    with gs.DegreeStream("all", vertex_hint=16) as D:
        for lo, hi in ((0, len(src)),) if cut is None else ((0, cut), (cut, len(src))):
            D.fold(src[lo:hi], dst[lo:hi], dele[lo:hi])
            _, d, c = D.records()
            got += ["(%d,%d)" % (a, b) for a, b in zip(d.tolist(), c.tolist())]
    assert got == pins[result]["text"].split("\n")


# ---------------------------------------------------------------- shapes
def _shape(name, m, T, rng):
    """(prelude, fold): occurrence lists (vertices, signs); the prelude fixes the ranks and seeds."""
    none = ([], [])
    if name == "own_segments":
        return none, (rng.permutation(m) * 3 - m, np.ones(m, int))
    if name == "one_vertex":
        return none, (np.full(m, 7), rng.choice([1, 1, -1], m))
    if name == "head_at_tile_first":  # A fills a tile exactly, B's head is the next tile's first
        seg = ([11] * T + [22] * (T + 3) + [33] * (2 * T))[:m]
        return ([11, 22, 33], [1, 1, 1]), (rng.permutation(seg), rng.choice([1, 1, -1], m))
    if name == "head_at_tile_last":  # B's head is a tile's last element and its segment goes on
        seg = ([11] * (T - 1) + [22] * (T + 1) + [33] * (2 * T))[:m]
        return ([11, 22, 33], [1, 1, 1]), (rng.permutation(seg), rng.choice([1, 1, -1], m))
    if name == "clamp_carried":  # a hub taken to 0 in the first tile, forgotten deletions, then additions
        k = m // 2 if m <= T else T + (m - T + 1) // 2  # past the first tile whenever there is a second
        return ([5] * 5, [1] * 5), (np.full(m, 5), np.array([-1] * k + [1] * (m - k)))
    if name == "never_seen_deletion":
        v = rng.integers(0, max(2, m // 3), m)
        s = np.ones(m, int)
        s[: (m + 1) // 2] = -1  # the first half deletes vertices nobody added
        return none, (v, s)
    if name == "extreme_ids":
        return none, (rng.choice([I64_MIN, I64_MAX - FAR, -1, 0], m), rng.choice([1, 1, -1], m))
    raise KeyError(name)


SHAPES = ("own_segments", "one_vertex", "head_at_tile_first", "head_at_tile_last", "clamp_carried",
          "never_seen_deletion", "extreme_ids")


@pytest.mark.parametrize("name", SHAPES)
def test_shapes_at_every_size(gs, name):
    T = gs.DEGSTREAM_TILE
    rng = np.random.default_rng(0xD5 + SHAPES.index(name))
    with gs.DegreeStream("out", vertex_hint=16) as D:
        for m in _sizes(gs):
            D.reset()
            M = Model("out")
            (pv, ps), (v, s) = _shape(name, m, T, rng)
            if len(pv):
                _fold_both(D, M, *_out_edges(pv, ps))
            rows, _ = _fold_both(D, M, *_out_edges(v, s))
            st = D.stats()
            assert st["tiles"] == (m + T - 1) // T
            if name == "one_vertex" and m > T:
                assert st["crossed"] >= (m - 1) // T  # one segment spans every tile
            if name == "own_segments":
                assert st["crossed"] == (m - 1) // T  # none by vertex; the records' one degree-1 segment
            if name == "clamp_carried" and m > T:
                assert any(o == 0 and n == 0 for _, o, n in rows[T:])  # forgotten past the first tile


def test_extreme_ids_under_all(gs):
    ids = np.array([I64_MIN, I64_MAX, -1, 0], np.int64)
    rng = np.random.default_rng(5)
    src, dst = rng.choice(ids, 300), rng.choice(ids, 300)
    with gs.DegreeStream("all", vertex_hint=16) as D:
        _fold_both(D, Model("all"), src, dst, rng.integers(0, 2, 300))


@pytest.mark.parametrize("direction", DIRS)
def test_self_loops(gs, direction):
    rng = np.random.default_rng(17)
    T = gs.DEGSTREAM_TILE
    n = T // 2 + 7
    src = rng.integers(0, 9, n)
    dst = np.where(rng.integers(0, 3, n) == 0, rng.integers(0, 9, n), src)  # two in three are loops
    dele = (rng.integers(0, 4, n) == 0).astype(np.uint8) | 2  # (bit 0 alone is read)
    with gs.DegreeStream(direction, vertex_hint=16) as D:
        rows, _ = _fold_both(D, Model(direction), src, dst, dele)
        assert len(rows) == (2 * n if direction == "all" else n)


def test_never_seen_deletion_has_no_later_effect(gs):
    with gs.DegreeStream("all", vertex_hint=16) as D:
        M = Model("all")
        rows, recs = _fold_both(D, M, [1], [2], [1])
        assert rows == [(1, 0, 0), (2, 0, 0)] and recs == []
        rows, recs = _fold_both(D, M, [1, 1], [2, 2], [0, 1])
        assert rows == [(1, 0, 1), (2, 0, 1), (1, 1, 0), (2, 1, 0)]
        assert recs == [(0, 1, 1), (1, 1, 2), (2, 1, 1), (3, 1, 0)]  # a count returns to 0 and is emitted as 0
        _fold_both(D, M, [1], [2])  # ... and rises again
        assert D.distribution()[1].tolist() == [2]


# ---------------------------------------------------------------- record side
def test_long_same_degree_segment(gs):
    T = gs.DEGSTREAM_TILE
    m = 3 * T + 5
    with gs.DegreeStream("out", vertex_hint=16) as D:
        v = np.arange(m, dtype=np.int64) * 7 - 100
        D.fold(v, v + FAR)
        o, d, c = D.records()
        assert np.array_equal(o, np.arange(m)) and np.all(d == 1) and np.array_equal(c, np.arange(1, m + 1))
        assert D.stats()["crossed"] == 3  # the one degree-1 segment crosses every record tile
        assert D.distribution()[0].tolist() == [1] and D.distribution()[1].tolist() == [m]


def test_star_grows_the_count_array(gs):
    k = gs.DEGSTREAM_MIN_COUNTS + 40
    with gs.DegreeStream("all", vertex_hint=16) as D:
        M = Model("all")
        assert D.stats()["count_capacity"] == gs.DEGSTREAM_MIN_COUNTS and D.stats()["count_growths"] == 0
        leaves = np.arange(1, k + 1, dtype=np.int64)
        _fold_both(D, M, np.zeros(k // 2, np.int64), leaves[: k // 2])
        assert D.stats()["count_growths"] == 0
        _fold_both(D, M, np.zeros(k - k // 2, np.int64), leaves[k // 2:])  # the centre passes the first capacity
        st = D.stats()
        assert st["count_growths"] == 1 and st["count_capacity"] == 2 * gs.DEGSTREAM_MIN_COUNTS
        assert D.size()["max_degree"] == k
        assert M.distribution() == [(1, k), (k, 1)]
        _fold_both(D, M, np.zeros(3, np.int64), leaves[:3], [1, 1, 1])


# ---------------------------------------------------------------- state across calls
def _stream(rng, n, vertices):
    src, dst = rng.integers(0, vertices, n), rng.integers(0, vertices, n)
    dst = np.where(rng.integers(0, 8, n) == 0, src, dst)
    return src.astype(np.int64), dst.astype(np.int64), (rng.integers(0, 3, n) == 0).astype(np.uint8)


def test_cuts_do_not_change_rows_or_records(gs):
    T = gs.DEGSTREAM_TILE
    rng = np.random.default_rng(0xC07)
    n = 2 * T + 77
    src, dst, dele = _stream(rng, n, 200)
    M = Model("all")
    rows, recs = M.fold(src, dst, dele)
    with gs.DegreeStream("all", vertex_hint=16) as D:
        for cut in (None, 1, T - 1, T, int(rng.integers(2, n - 1))):
            D.reset()
            got_rows, got_recs, base = [], [], 0
            for lo, hi in ((0, n),) if cut is None else ((0, cut), (cut, n)):
                D.fold(src[lo:hi], dst[lo:hi], dele[lo:hi])
                r, c = _got(D)
                got_rows += r
                got_recs += [(o + base, d, k) for o, d, k in c]
                base += 2 * (hi - lo)
            assert got_rows == rows and got_recs == recs, cut
            _check_state(D, M)


def test_vertex_table_grows_between_folds(gs):
    rng = np.random.default_rng(3)
    with gs.DegreeStream("all", vertex_hint=0) as D:
        M = Model("all")
        before = gs.hbm_bytes(0)
        for k in range(3):  # 4096 distinct ids per fold: past the smallest table's 512 ranks at once
            ids = np.arange(k * 4096, (k + 1) * 4096, dtype=np.int64) * 5
            src = np.concatenate([ids, rng.choice(ids, 100)])
            _fold_both(D, M, src, src[::-1].copy(), (rng.integers(0, 5, len(src)) == 0).astype(np.uint8))
        assert gs.hbm_bytes(0) > before
        assert len(D.degrees()[0]) == len(M.degrees()) > 4096


def test_reset_and_empty_fold(gs):
    with gs.DegreeStream("all", vertex_hint=16) as D:
        M = Model("all")
        D.fold([], [])
        assert D.size() == {"vertices": 0, "occurrences": 0, "records": 0, "total": 0, "max_degree": 0}
        assert _got(D) == ([], []) and len(D.degrees()[0]) == 0 and len(D.distribution()[0]) == 0
        _fold_both(D, M, [1, 2, 3], [2, 3, 1])
        D.fold([], [], [])
        assert _got(D) == ([], [])  # the last fold had no rows
        _check_state(D, M)
        D.reset()
        assert D.size()["total"] == 0 and len(D.degrees()[0]) == 0 and len(D.distribution()[0]) == 0
        _fold_both(D, Model("all"), [1, 2, 3], [2, 3, 1])


def test_device_folds_and_reads_with_sentinels(gs):
    import torch
    rng = np.random.default_rng(9)
    n = 700
    src, dst, dele = _stream(rng, n, 50)
    dev = torch.device("cuda", 0)
    with gs.DegreeStream("all", vertex_hint=16) as D:
        M = Model("all")
        rows, recs = M.fold(src, dst, dele)
        # strided device arrays: element i at index 2 i
        ts = torch.from_numpy(np.repeat(src, 2)).to(dev)
        td = torch.from_numpy(np.repeat(dst, 2)).to(dev)
        te = torch.from_numpy(dele).to(dev)
        D.fold_device(ts, td, n=n, stride=2, deletions=te, after="torch")
        D.sync()
        assert _got(D) == (rows, recs)
        m, r = len(rows), len(recs)
        tv = torch.full((m + 1,), SENTINEL, dtype=torch.int64, device=dev)
        to, tn = (torch.full((m + 1,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2))
        ra, rb, rc = (torch.full((r + 1,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3))
        D.wait_stream("torch")
        assert D.rows_device(tv, to, tn) == m and D.records_device(ra, rb, rc) == r
        D.sync()
        assert list(zip(tv[:m].tolist(), to[:m].tolist(), tn[:m].tolist())) == rows
        assert list(zip(ra[:r].tolist(), rb[:r].tolist(), rc[:r].tolist())) == recs
        for t in (tv, to, tn, ra, rb, rc):
            assert int(t[-1]) == SENTINEL
        nd, ng = len(M.degrees()), len(M.distribution())
        dv, dd = (torch.full((nd + 1,), SENTINEL, dtype=torch.int64, device=dev) for _ in range(2))
        gd, gc = (torch.full((ng + 1,), SENTINEL, dtype=torch.int64, device=dev) for _ in range(2))
        D.wait_stream("torch")
        assert D.degrees_device(dv, dd) == nd and D.distribution_device(gd, gc) == ng
        D.sync()
        assert sorted(zip(dv[:nd].tolist(), dd[:nd].tolist())) == M.degrees()
        assert list(zip(gd[:ng].tolist(), gc[:ng].tolist())) == M.distribution()
        for t in (dv, dd, gd, gc):
            assert int(t[-1]) == SENTINEL
        # a too small array: the count, nothing written
        small = torch.full((3,), SENTINEL, dtype=torch.int64, device=dev)
        with pytest.raises(gs.GSError) as e:
            D.rows_device(small, None, None)
        assert e.value.code == gs.GS_ERR_TRUNCATED
        D.sync()
        assert small.tolist() == [SENTINEL] * 3


def test_a_fold_longer_than_the_largest_kept_one_is_cut_by_the_library(gs):
    """DEGSTREAM_MAX_FOLD + 5 device edges, additions only, so that the truth is a bincount: the
    state is that of one fold, the sizes are the sums over the pieces, the rows are not kept, and
    the next short fold keeps its rows again."""
    import torch
    dev = torch.device("cuda", 0)
    n, ids = gs.DEGSTREAM_MAX_FOLD + 5, 1000
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    src = torch.randint(0, ids, (n,), dtype=torch.int64, device=dev, generator=g)
    dst = torch.randint(0, ids, (n,), dtype=torch.int64, device=dev, generator=g)
    want = (torch.bincount(src, minlength=ids) + torch.bincount(dst, minlength=ids)).cpu().numpy()
    with gs.DegreeStream("all", vertex_hint=ids) as D:
        D.fold_device(src, dst, after="torch")
        D.sync()
        v, d = D.degrees()
        assert np.array_equal(v, np.arange(ids)) and np.array_equal(d, want)
        k, c = D.distribution()
        uk, uc = np.unique(want, return_counts=True)
        assert np.array_equal(k, uk) and np.array_equal(c, uc)
        s = D.size()
        # an addition gives one record at a vertex's first occurrence and two at every later one
        assert (s["vertices"], s["occurrences"], s["records"], s["total"]) == (ids, 2 * n, 4 * n - ids, 2 * n)
        assert s["max_degree"] == want.max()
        for read in (D.rows, D.records):
            with pytest.raises(gs.GSError) as e:
                read()
            assert e.value.code == gs.GS_ERR_INVALID
        D.fold([1], [2])
        assert D.rows()[0].tolist() == [1, 2] and len(D.records()[0]) == 4


def test_overflow_rule_fails_before_any_work(gs):
    import ctypes
    with gs.DegreeStream("all", vertex_hint=16) as D:
        D.fold([1], [2])
        # 2^30 edges under ALL are 2^31 occurrences: refused from the count alone (the arrays are never read)
        one = np.zeros(1, np.int64)
        rc = gs.lib().gs_degstream_fold(D.handle, one.ctypes.data, one.ctypes.data, None, ctypes.c_size_t(1 << 30))
        assert rc == gs.GS_ERR_CAPACITY
        assert D.size()["total"] == 2 and D.rows()[0].tolist() == [1, 2]


# ---------------------------------------------------------------- agreement with the degree summary
def test_agrees_with_the_degree_summary_when_deletions_remove_present_edges(gs):
    rng = np.random.default_rng(0xA9)
    src, dst, _ = _stream(rng, 3000, 300)
    # delete only edges that are present: a random subset of the additions, after them
    pick = rng.permutation(3000)[:900]
    s = np.concatenate([src, src[pick]])
    d = np.concatenate([dst, dst[pick]])
    e = np.concatenate([np.zeros(3000, np.uint8), np.ones(900, np.uint8)])
    for direction in DIRS:
        with gs.DegreeStream(direction, vertex_hint=16) as D, gs.Degrees(direction, capacity_hint=1 << 10) as G:
            for lo in range(0, len(s), 1300):
                D.fold(s[lo:lo + 1300], d[lo:lo + 1300], e[lo:lo + 1300])
                G.fold(s[lo:lo + 1300], d[lo:lo + 1300], e[lo:lo + 1300])
            for a, b in zip(D.degrees(), G.degrees(sorted=True)):
                assert np.array_equal(a, b)
            for a, b in zip(D.distribution(), G.distribution()):
                assert np.array_equal(a, b)


def test_differs_from_the_degree_summary_on_a_deletion_of_an_absent_edge(gs):
    # 1-2 deleted before it ever arrives, then added: the reference (and the stream) forget the
    # deletion, the degree summary keeps it in the net count
    s, d, e = [1, 1, 3], [2, 2, 4], [1, 0, 0]
    with gs.DegreeStream("all", vertex_hint=16) as D, gs.Degrees("all", capacity_hint=1 << 10) as G:
        D.fold(s, d, e)
        G.fold(s, d, e)
        assert [x.tolist() for x in D.degrees()] == [[1, 2, 3, 4], [1, 1, 1, 1]]
        assert [x.tolist() for x in G.degrees(sorted=True)] == [[3, 4], [1, 1]]
        assert [x.tolist() for x in D.distribution()] == [[1], [4]]
        assert [x.tolist() for x in G.distribution()] == [[1], [2]]
