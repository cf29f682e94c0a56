"""GPU: the k-spanner summary at the shapes its kernels branch on ("Tested").

1. the distance boundary -- a path of k or k + 1 edges closed by one arrival -- for every k in
   1..16, with fans of 0, 3 and 70 leaves at either end and in the middle (lopsided frontiers),
   decided by the filter pass, by rounds, by the tail, on rows that are part adjacency and part
   pending, and on the heavy path;
2. decision chains (ladders) on which every round decides exactly one edge: the device's round
   and tail counts equal Model.fold_rounds, the restatement of SpannerSeq::fold_rounds;
3. a hub whose row is part adjacency, part pending, up to 600 entries;
4. loops and their dead second entries among pending entries;
5. the three compactions (pending edges, accepted entries, export) at SPANNER_TILE +- 1 and one
   tile count past a step of the tile-count scan;
6. the stamp arenas across every clear: generation run-out, pool regrow, arena-count change.

Truth is test_gpu_spanner.Model throughout; every comparison is exact. The generators are plain
Python over dense ids and are checked on the CPU in test_spanner_shapes.py."""
import contextlib
import functools

import numpy as np
import pytest

from test_gpu_spanner import INT64_MIN, Model, _edges_of, _scramble

pytestmark = pytest.mark.gpu

HUGE = 1 << 40
STAT_KEYS = ("filter_drops", "pending", "rounds", "tail")


def _ids(n, salt, special):
    """n sparse signed ids; dense vertex `special`, one that matters to the case, is INT64_MIN."""
    with np.errstate(over="ignore"):
        ids = _scramble(np.arange(n), salt)
    ids[special] = INT64_MIN
    assert len(np.unique(ids)) == n and (ids < 0).sum() > 1
    return ids


def _arrays(ids, pairs):
    e = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    return ids[e[:, 0]], ids[e[:, 1]]


def _check_export(sp, model):
    """The export of the device graph is the model's graph: the merge writes entries by computed
    position, so an entry written twice or never shows here and nowhere else."""
    want = model.edges()
    assert _edges_of(sp) == want
    assert sp.count() == (len(want), len(model.adj))
    v, off, nb = sp.neighbors()
    assert len(v) == len(model.adj) and (np.diff(v) > 0).all()
    assert off[0] == 0 and off[-1] == len(nb) and len(off) == len(v) + 1
    rows = {x: nb[off[i]:off[i + 1]].tolist() for i, x in enumerate(v.tolist())}
    for x, row in rows.items():
        assert all(a < b for a, b in zip(row, row[1:])), x  # ascending, so a loop is there once
        assert all(x in rows[y] for y in row), x  # symmetric
    assert rows == {x: sorted(r) for x, r in model.adj.items()}


def _expect(k, folds, cap):
    """Model.fold_rounds over the folds: (mask, the folds' stats, the model afterwards)."""
    model, masks, stats = Model(k), [], []
    for src, dst in folds:
        mask, rounds, tail, drops = model.fold_rounds(src.tolist(), dst.tolist(), cap)
        masks.append(mask)
        stats.append({"filter_drops": drops, "pending": len(mask) - drops, "rounds": rounds, "tail": tail})
    return np.array([m for mask in masks for m in mask], dtype=bool), stats, model


def _fold_all(sp, folds, between=None):
    """Fold the folds into sp; returns (mask, stats of each fold). between(sp): after the first."""
    masks, stats = [], []
    for i, (src, dst) in enumerate(folds):
        masks.append(sp.fold(src, dst))
        stats.append(sp.stats())
        if i == 0 and between:
            between(sp)
    return np.concatenate(masks), stats


def _same_stats(got, want, what):
    assert [{key: s[key] for key in STAT_KEYS} for s in got] == want, what


# ---------------------------------------------------------------- 1. the distance boundary
FANS = (0, 3, 70)  # 70: more than the 64 lanes that stride a row, fewer than the 256 of an on-chip set


def fan_path(L, fs, ft, fm):
    """Dense ids: a path 0 - 1 - ... - L with fs leaves at s = 0, ft at t = L and fm at the middle
    vertex L // 2. Returns (body edges: the path, then the leaves hub by hub, each leaf named
    first; the closing arrival (s, t); vertices; a leaf at s or None). The body is a tree in
    which s and t are exactly L apart."""
    body = [(v, v + 1) for v in range(L)]
    n = L + 1
    for hub, f in ((0, fs), (L, ft), (L // 2, fm)):
        for _ in range(f):
            body.append((n, hub))
            n += 1
    return body, (0, L), n, L + 1 if fs else None


@functools.lru_cache(maxsize=None)
def fan_stream(k):
    """The 54 cases of k -- L in (k, k + 1) x fans in FANS^3 -- as disjoint components of one
    stream. Returns a dict: cases (their tuple, s, t, leaf at s, as ids), body and closers as id
    arrays with the case index of every arrival and the position of a body edge in its case;
    closers alternate their orientation."""
    cases, body, closers, owner, pos, base = [], [], [], [], [], 0
    for L in (k, k + 1):
        for fs in FANS:
            for ft in FANS:
                for fm in FANS:
                    b, (s, t), n, leaf = fan_path(L, fs, ft, fm)
                    c = len(cases)
                    cases.append({"case": (L, fs, ft, fm), "s": base + s, "t": base + t,
                                  "leaf": None if leaf is None else base + leaf})
                    body += [(base + u, base + v) for u, v in b]
                    owner += [c] * len(b)
                    pos += range(len(b))
                    closers.append((base + t, base + s) if c % 2 else (base + s, base + t))
                    base += n
    special = next(c["s"] for c in cases if c["case"] == (k, 70, 3, 70))  # a path endpoint and hub
    ids = _ids(base, 100 + k, special)
    for c in cases:
        for key in ("s", "t", "leaf"):
            c[key] = None if c[key] is None else int(ids[c[key]])
    return {"cases": cases, "body": _arrays(ids, body), "closers": _arrays(ids, closers),
            "body_owner": np.array(owner), "body_pos": np.array(pos), "vertices": base}


@functools.lru_cache(maxsize=None)
def fan_folds(k, route):
    """(folds, case index of every arrival) of a route: "two" -- the body, then the closers;
    "one" -- both in one fold; "mixed" -- the even-indexed body edges of every case, then the odd
    ones and the closers, so that every path vertex and hub has a row part adjacency, part pending."""
    st = fan_stream(k)
    (bs, bd), (cs, cd) = st["body"], st["closers"]
    closer_owner = np.arange(len(cs))
    if route == "two":
        return ((bs, bd), (cs, cd)), np.concatenate([st["body_owner"], closer_owner])
    if route == "one":
        return ((np.concatenate([bs, cs]), np.concatenate([bd, cd])),), np.concatenate([st["body_owner"], closer_owner])
    even = st["body_pos"] % 2 == 0
    folds = ((bs[even], bd[even]), (np.concatenate([bs[~even], cs]), np.concatenate([bd[~even], cd])))
    return folds, np.concatenate([st["body_owner"][even], st["body_owner"][~even], closer_owner])


@functools.lru_cache(maxsize=None)
def fan_expect(k, route, cap=None):
    return _expect(k, fan_folds(k, route)[0], cap)


def _run_fan(gs, k, route, cap=None, between=None, heavy=False):
    folds, owner = fan_folds(k, route)
    want, want_stats, model = fan_expect(k, route, cap)
    cases = fan_stream(k)["cases"]
    with gs.testing(spanner_round_cap=cap), gs.Spanner(k=k, edge_hint=16) as sp:
        mask, stats = _fold_all(sp, folds, between)
        bad = np.flatnonzero(mask != want)
        assert bad.size == 0, (k, route, cap, [cases[owner[i]]["case"] for i in bad[:6]])
        _same_stats(stats, want_stats, (k, route, cap))
        if heavy:
            assert sum(s["heavy"] for s in stats) > 0
        _check_export(sp, model)


KS = tuple(range(1, 17))


@pytest.mark.parametrize("k", KS)
def test_fan_body_then_closers(gs, k):
    """The filter pass decides every closer against G0, and between the folds within() has the
    boundary at exactly L for every k' in 1..16."""
    cases = fan_stream(k)["cases"]

    def between(sp):
        by_k = {}  # query k' -> [(s, t, want, case)]
        for c in cases:
            L = c["case"][0]
            for kq, s, t, want in ((L - 1, c["s"], c["t"], False), (L, c["s"], c["t"], True),
                                   (L + 1, c["leaf"], c["t"], True)):
                if 1 <= kq <= 16 and s is not None:
                    by_k.setdefault(kq, []).append((s, t, want, c["case"]))
        assert len(by_k) >= 2
        for kq, qs in by_k.items():
            got = sp.within([q[0] for q in qs], [q[1] for q in qs], kq).tolist()
            bad = [(kq, q[3]) for q, g in zip(qs, got) if g != q[2]]
            assert not bad, (k, bad[:6])

    _run_fan(gs, k, "two", between=between)


@pytest.mark.parametrize("cap", (None, 0, HUGE))
@pytest.mark.parametrize("k", KS)
def test_fan_one_fold(gs, k, cap):
    """Body and closers in one fold: by rounds (product), by the tail alone (cap 0: every search a
    lower search on arena 0), by rounds alone (a huge cap)."""
    _run_fan(gs, k, "one", cap)
    if cap == 0:
        assert fan_expect(k, "one", 0)[1][0]["tail"] == fan_expect(k, "one", 0)[1][0]["pending"] > 0
    if cap == HUGE:
        assert fan_expect(k, "one", HUGE)[1][0]["tail"] == 0


@pytest.mark.parametrize("k", KS)
def test_fan_mixed_rows(gs, k):
    _run_fan(gs, k, "mixed")


@pytest.mark.parametrize("arenas", (None, 1))
@pytest.mark.parametrize("route", ("one", "mixed"))
@pytest.mark.parametrize("k", KS)
def test_fan_heavy_path(gs, k, route, arenas):
    with gs.testing(spanner_lds_set=2, spanner_arenas=arenas):
        _run_fan(gs, k, route, heavy=True)


# ---------------------------------------------------------------- 2. decision chains
def ladder(k, rungs, p):
    """Dense ids: rail A = a path on which consecutive rung ends are p edges apart (p = 0: one
    vertex), rail B the same with k - 1 - p. Rung i joins the i-th rung ends; from one end to the
    other it is k edges by way of rung i - 1 and 2 k - 1 by way of rung i - 2, so rung i is within
    k iff rung i - 1 is in the graph: the verdicts alternate, accepted first. Returns (rail
    edges, rungs in arrival order with alternating orientation, vertices)."""
    q = k - 1 - p
    assert k >= 2 and 0 <= p <= k - 1
    na, nb = p * (rungs - 1) + 1, q * (rungs - 1) + 1
    rails = [(v, v + 1) for v in range(na - 1)] + [(na + v + 1, na + v) for v in range(nb - 1)]
    rung = [(i * p, na + i * q) if i % 2 == 0 else (na + i * q, i * p) for i in range(rungs)]
    return rails, rung, na + nb


LADDERS = tuple((k, p) for k in (2, 3, 16) for p in sorted({0, (k - 1) // 2, k - 1}))
RUNGS = 40


@functools.lru_cache(maxsize=None)
def ladder_folds(k, rungs, p, same_fold):
    rails, rung, n = ladder(k, rungs, p)
    ids = _ids(n, 200 + 16 * k + p, p)  # a_1, a rung end
    if same_fold:
        return (_arrays(ids, rails + rung),)
    return _arrays(ids, rails), _arrays(ids, rung)


@functools.lru_cache(maxsize=None)
def ladder_expect(k, rungs, p, same_fold, cap):
    return _expect(k, ladder_folds(k, rungs, p, same_fold), cap)


def _run_ladder(gs, k, rungs, p, same_fold, cap):
    folds = ladder_folds(k, rungs, p, same_fold)
    want, want_stats, model = ladder_expect(k, rungs, p, same_fold, cap)
    with gs.Spanner(k=k, edge_hint=16) as sp:
        masks, stats = [], []
        for i, (src, dst) in enumerate(folds):
            with gs.testing(spanner_round_cap=cap) if i == len(folds) - 1 else contextlib.nullcontext():
                masks.append(sp.fold(src, dst))
            stats.append(sp.stats())
        assert np.array_equal(np.concatenate(masks), want), (k, p, cap)
        if not same_fold:
            assert stats[-1]["pending"] == rungs and masks[-1].tolist() == [i % 2 == 0 for i in range(rungs)]
        _same_stats(stats[-1:], want_stats[-1:], (k, p, cap, stats[-1]))
        _check_export(sp, model)
    return stats[-1]


@pytest.mark.parametrize("k,p", LADDERS)
def test_ladder_rounds_and_tail_equal_the_restatement(gs, k, p):
    """Rails in an earlier fold: every round decides exactly one rung, and a round that read a
    status of its own launch, or the tail one not yet written, would decide more or otherwise."""
    for cap in (None, 0, 1, 3, HUGE):
        st = _run_ladder(gs, k, RUNGS, p, False, cap)
        rounds = {None: 1, 0: 0, 1: 1, 3: 3, HUGE: RUNGS}[cap]  # (product: 1 of 40 is slow progress)
        assert (st["rounds"], st["tail"]) == (rounds, RUNGS - rounds), cap


@pytest.mark.parametrize("k,p", LADDERS)
def test_ladder_with_its_rails_in_the_same_fold(gs, k, p):
    for cap in (None, HUGE):
        st = _run_ladder(gs, k, RUNGS, p, True, cap)
        # round 1 takes the rails and rung 0; under the product rule round 2, one rung of 39, is the last
        assert (st["rounds"], st["tail"]) == ((2, RUNGS - 2) if cap is None else (RUNGS, 0)), cap


@pytest.mark.parametrize("lds_set", (None, 2))
def test_long_ladder_tail_spans_two_chunks(gs, lds_set):
    """300 undecided statuses: the tail reads them 256 at a time, undecided bytes in both chunks."""
    with gs.testing(spanner_lds_set=lds_set):
        st = _run_ladder(gs, 3, 300, 1, False, 0)
    assert (st["rounds"], st["tail"], st["pending"]) == (0, 300, 300)


# ---------------------------------------------------------------- 3. a hub row, part adjacency, part pending
@functools.lru_cache(maxsize=None)
def hub_folds(a, b):
    """Centre 0 with leaves 1..a folded first; the second fold interleaves the spokes of the new
    leaves a + 1..a + b with arrivals between old leaves, between an old and a new one, and
    between new ones -- some of them before their leaf's spoke."""
    old = lambda i: 1 + i % a
    new = lambda i: a + 1 + i
    first = [(0, old(i)) for i in range(a)]
    second = []
    for i in range(b):
        if i % 4 == 3:
            second.append((new(i), old(3 * i)))  # before new(i)'s spoke
        second.append((0, new(i)) if i % 2 == 0 else (new(i), 0))
        if i % 3 == 0:
            second.append((old(i), old(i + 1)))
        if i % 4 == 1:
            second.append((old(2 * i), new(i)))
        if i % 2 == 0 and i > 0:
            second.append((new(i), new(i - 1)))
        if i % 5 == 0 and i + 1 < b:
            second.append((new(i + 1), new(i)))  # before new(i + 1)'s spoke
    ids = _ids(a + b + 1, 300 + a, 0)  # the hub
    return _arrays(ids, first), _arrays(ids, second)


@functools.lru_cache(maxsize=None)
def hub_expect(a, b, k):
    model = Model(k)
    return tuple(np.array(model.fold(s.tolist(), d.tolist()), dtype=bool) for s, d in hub_folds(a, b)), model


HUBS = ((40, 40), (100, 100), (300, 300))


@pytest.mark.parametrize("knobs", ({}, {"spanner_round_cap": 0}, {"spanner_arenas": 1}), ids=("product", "cap0", "arena1"))
@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("a,b", HUBS)
def test_hub_row_part_adjacency_part_pending(gs, a, b, k, knobs):
    folds = hub_folds(a, b)
    want, model = hub_expect(a, b, k)
    with gs.testing(**knobs), gs.Spanner(k=k, edge_hint=16) as sp:
        mask, stats = _fold_all(sp, folds)
        assert np.array_equal(mask, np.concatenate(want)), (a, b, k, np.flatnonzero(mask != np.concatenate(want))[:8])
        assert all(s["filter_drops"] + s["pending"] == len(f[0]) for s, f in zip(stats, folds))
        if (a, b) == (300, 300):  # past the on-chip set: 256 threads walk the row
            assert stats[1]["heavy"] > 0 and stats[1]["longest_row"] >= 600
        _check_export(sp, model)


# ---------------------------------------------------------------- 4. loops and dead entries
@functools.lru_cache(maxsize=None)
def loop_stream():
    """A path of 10 vertices: its edges, their reversed duplicates and a loop at every vertex
    arriving twice, interleaved. Returns (ids, src, dst)."""
    pairs = []
    for v in range(10):
        pairs.append((v, v))
        if v < 9:
            pairs += [(v, v + 1), (v + 1, v)]
        pairs.append((v, v))
    ids = _ids(10, 400, 0)  # a path endpoint
    return (ids,) + _arrays(ids, pairs)


@pytest.mark.parametrize("batch", (1, 3, None))
@pytest.mark.parametrize("k", (1, 2))
def test_loops_among_pending_entries(gs, k, batch):
    ids, src, dst = loop_stream()
    batch = batch or len(src)
    model = Model(k)
    want = model.fold(src.tolist(), dst.tolist())
    assert sum(want) == 19  # every loop and path edge once
    with gs.Spanner(k=k, edge_hint=16) as sp:
        got = np.concatenate([sp.fold(src[i:i + batch], dst[i:i + batch]) for i in range(0, len(src), batch)])
        assert got.tolist() == want
        _check_export(sp, model)
        stranger = np.int64(12345)
        assert stranger not in ids
        q = np.concatenate([ids, [stranger]])
        for kq in (1, 16):
            assert sp.within(q, q, kq).tolist() == [True] * 10 + [False]
        sp.reset()  # a path without loops: within(v, v) is false however close the neighbours are
        sp.fold(ids[:-1], ids[1:])
        assert not sp.within(q, q, 16).any()


# ---------------------------------------------------------------- 5. tiles of the three compactions
def tile_pairs(n, salt=500):
    """n disjoint edges (id(2 i), id(2 i + 1)) as id arrays; id(0) is INT64_MIN."""
    ids = _ids(2 * n, salt, 0)
    return ids[0::2].copy(), ids[1::2].copy()


def tile_subsets(n, T):
    """name -> prefilled mask over the n edges"""
    i = np.arange(n)
    return {"none": i < 0, "all": i >= 0, "even": i % 2 == 0, "tile_last": i % T == T - 1, "tile_first": i % T == 0,
            "all_but_last": i < n - 1}


def tile_expect(src, dst, pre):
    """The closed form: (mask, stats, sorted (lo, hi) arrays) of folding all n over the prefilled."""
    n, filled = len(src), int(pre.sum())
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    order = np.lexsort((hi, lo))
    stats = {"filter_drops": filled, "pending": n - filled, "rounds": 1 if n > filled else 0, "tail": 0}
    return ~pre, stats, lo[order], hi[order]


def _tile_sizes(gs):
    T = gs.SPANNER_TILE
    return T, (T - 1, T, T + 1, 2 * T, 2 * T + 1)


@pytest.mark.parametrize("which", range(5))
def test_tiles_at_the_tile_size(gs, which):
    T, sizes = _tile_sizes(gs)
    n = sizes[which]
    src, dst = tile_pairs(n)
    model = Model(3)
    for s, t in zip(src.tolist(), dst.tolist()):
        model.add(s, t)
    for name, pre in tile_subsets(n, T).items():
        want, want_stats, lo, hi = tile_expect(src, dst, pre)
        with gs.Spanner(k=3, edge_hint=16) as sp:
            if pre.any():
                sp.add(src[pre], dst[pre])
                assert sp.count() == (int(pre.sum()), 2 * int(pre.sum())), name
            got = sp.fold(src, dst)
            assert np.array_equal(got, want), (n, name, np.flatnonzero(got != want)[:8])
            _same_stats([sp.stats()], [want_stats], (n, name))
            assert sp.count() == (n, 2 * n), (n, name)
            glo, ghi = sp.edges()
            assert np.array_equal(glo, lo) and np.array_equal(ghi, hi), (n, name)
            _check_export(sp, model)


def test_tiles_combine_from_an_export_of_several_tiles(gs):
    T = gs.SPANNER_TILE
    n = 2 * T + 1
    src, dst = tile_pairs(n)
    _, _, lo, hi = tile_expect(src, dst, np.zeros(n, bool))
    with gs.Spanner(k=3, edge_hint=16) as full, gs.Spanner(k=3, edge_hint=16) as half:
        full.add(src, dst)
        half.add(src[::2], dst[::2])
        half.combine(full)
        st = half.stats()
        assert (st["filter_drops"], st["pending"], st["rounds"], st["tail"]) == (T + 1, T, 1, 0)
        assert half.count() == full.count() == (n, 2 * n)
        for sp in (half, full):
            glo, ghi = sp.edges()
            assert np.array_equal(glo, lo) and np.array_equal(ghi, hi)


def test_tiles_past_one_step_of_the_tile_scan(gs):
    """TILE_SCAN_BLOCK * T + 1 arrivals, a third prefilled: 1025 tile counts for the pending
    compaction, more than 1024 for the accepted entries and 2049 for the export -- each scan
    carries a sum out of its first step."""
    T = gs.SPANNER_TILE
    n = gs.TILE_SCAN_BLOCK * T + 1
    src, dst = tile_pairs(n, 501)
    pre = np.arange(n) % 3 == 0
    want, want_stats, lo, hi = tile_expect(src, dst, pre)
    assert -(-n // T) == gs.TILE_SCAN_BLOCK + 1 and 2 * want_stats["pending"] > gs.TILE_SCAN_BLOCK * T
    with gs.Spanner(k=3, edge_hint=16) as sp:
        sp.add(src[pre], dst[pre])
        got = sp.fold(src, dst)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        _same_stats([sp.stats()], [want_stats], n)
        assert sp.count() == (n, 2 * n)
        glo, ghi = sp.edges()
        assert np.array_equal(glo, lo) and np.array_equal(ghi, hi)
        v, off, nb = sp.neighbors()  # every row is one entry: the other end
        ends = np.concatenate([src, dst])
        order = np.argsort(ends)
        assert np.array_equal(v, ends[order]) and np.array_equal(off, np.arange(2 * n + 1))
        assert np.array_equal(nb, np.concatenate([dst, src])[order])


# ---------------------------------------------------------------- 6. stamp arrays across their clears
@functools.lru_cache(maxsize=None)
def two_stars(leaves=8):
    """Dense: centres 0 and 1 joined by an edge, leaves 2.. alternately at either. Returns (ids,
    src, dst, a leaf of star A, a leaf of star B): the two leaves are exactly 3 apart."""
    pairs = [(0, 1)] + [(i % 2, 2 + i) for i in range(2 * leaves)]
    ids = _ids(2 + 2 * leaves, 600, 0)  # a hub
    return (ids,) + _arrays(ids, pairs) + (int(ids[2]), int(ids[3]))


def _star_queries(sp, la, lb):
    """Eight true and eight false searches, all of them heavy under spanner_lds_set=2."""
    return sp.within([la] * 8, [lb] * 8, 3).tolist() + sp.within([lb] * 8, [la] * 8, 2).tolist()


def _star_queries_last_true(sp, ids):
    """Fifteen false searches that never reach leaf `la`, then one true search from it: `la` is
    stamped once, with the last generation and its own side."""
    la, lb, la2 = int(ids[2]), int(ids[3]), int(ids[4])
    return sp.within([lb] * 15, [la2] * 15, 2).tolist() + sp.within([la], [lb], 3).tolist()


def test_stamps_survive_the_generation_running_out(gs):
    """Repeated queries restamp the vertices they share, so uncleared stamps go unnoticed by
    copies of one query; the sixteenth search below starts from a leaf the fifteen before it
    leave alone. On uncleared stamps its rerun, in generation 15 again, finds its own source
    stamped "mine" and answers false."""
    ids, src, dst, la, lb = two_stars()
    with gs.Spanner(k=3, edge_hint=16) as sp, contextlib.ExitStack() as knobs:
        assert sp.fold(src, dst).all() and sp.stats()["heavy"] == 0
        assert sp.generation() == 0  # no heavy search yet: the rerun below has generations 0..15 again
        knobs.enter_context(gs.testing(spanner_lds_set=2, spanner_arenas=1))
        assert _star_queries_last_true(sp, ids) == [False] * 15 + [True]
        assert sp.generation() == 16  # every query was a heavy search
        assert sp.generation(set=gs.SPANNER_MAX_GEN - 1) == gs.SPANNER_MAX_GEN - 1
        assert _star_queries_last_true(sp, ids) == [False] * 15 + [True]
        assert sp.generation() == 16  # cleared once, by the first of the two calls, and counted on
        # eight copies of a true and of a false query, before and after another clear
        assert _star_queries(sp, la, lb) == [True] * 8 + [False] * 8
        assert sp.generation() == 32
        assert sp.generation(set=1 << 40) == gs.SPANNER_MAX_GEN  # clamped
        assert _star_queries(sp, la, lb) == [True] * 8 + [False] * 8
        assert sp.generation() == 16 < 64
        with pytest.raises(gs.GSError) as e:
            gs._check(gs.lib().gs_testing_spanner_generation(sp._h, -1, None))
        assert e.value.code == gs.GS_ERR_INVALID


def test_stamps_survive_the_generation_running_out_in_a_fold(gs):
    want, want_stats, model = ladder_expect(3, RUNGS, 1, False, 0)
    (rs, rd), (us, ud) = ladder_folds(3, RUNGS, 1, False)
    for lds_set, bound in ((None, 64), (2, 128)):  # (2: the filter's 40 heavy searches take the clear)
        with gs.testing(spanner_lds_set=lds_set, spanner_arenas=1, spanner_round_cap=0), gs.Spanner(k=3, edge_hint=16) as sp:
            first = sp.fold(rs, rd)
            sp.generation(set=gs.SPANNER_MAX_GEN - 1)
            got = np.concatenate([first, sp.fold(us, ud)])
            assert np.array_equal(got, want), lds_set
            _same_stats([sp.stats()], want_stats[-1:], lds_set)
            assert RUNGS <= sp.generation() < bound  # the tail took 40 generations after the clear
            _check_export(sp, model)


def test_stamps_survive_a_pool_regrow(gs):
    ids, src, dst, la, lb = two_stars()
    n = 10 * len(src)
    with np.errstate(over="ignore"):
        more = _scramble(np.arange(2 * n), 601)
    assert not set(more.tolist()) & set(ids.tolist())
    cross = (np.array([la, lb, la]), np.array([lb, int(ids[4]), int(more[0])]))  # 3 apart; 3 apart; no path
    model = Model(2)
    with gs.testing(spanner_lds_set=2, spanner_arenas=1), gs.Spanner(k=2, edge_hint=16) as sp:
        assert sp.fold(src, dst).tolist() == model.fold(src.tolist(), dst.tolist())
        assert sp.stats()["heavy"] > 0 and sp.generation() > 0  # the pool is sized for this graph
        sp.add(more[0::2], more[1::2])
        for s, t in zip(more[0::2].tolist(), more[1::2].tolist()):
            model.add(s, t)
        assert sp.fold(*cross).tolist() == model.fold(cross[0].tolist(), cross[1].tolist()) == [True, True, True]
        assert sp.stats()["heavy"] > 0
        qs, qd = np.array([la, lb, la, int(more[1])]), np.array([int(ids[5]), la, int(more[0]), lb])
        for kq in (1, 2, 3, 16):
            want = [model.within(s, t, kq) for s, t in zip(qs.tolist(), qd.tolist())]
            assert sp.within(qs, qd, kq).tolist() == want, kq
        _check_export(sp, model)


def test_stamps_survive_a_change_of_the_arena_count(gs):
    src, dst = hub_folds(40, 40)[1]
    model = Model(2)
    with gs.testing(spanner_lds_set=2), gs.Spanner(k=2, edge_hint=16) as sp:
        cuts = np.linspace(0, len(src), 7).astype(int)
        for arenas, lo, hi in zip((1, 3, None, 1, None, 3), cuts[:-1], cuts[1:]):
            with gs.testing(spanner_arenas=arenas):
                got = sp.fold(src[lo:hi], dst[lo:hi]).tolist()
                assert got == model.fold(src[lo:hi].tolist(), dst[lo:hi].tolist()), arenas
                assert sp.stats()["heavy"] > 0, arenas
                q = sp.within(src[:hi], dst[:hi], 2).tolist()
                assert q == [model.within(s, t, 2) for s, t in zip(src[:hi].tolist(), dst[:hi].tolist())], arenas
        _check_export(sp, model)
