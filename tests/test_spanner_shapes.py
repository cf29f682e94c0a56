"""CPU: the generators of test_gpu_spanner_shapes.py do what the GPU tests rely on, and
Model.fold_rounds -- the Python restatement of SpannerSeq::fold_rounds those tests take their
round and tail counts from -- decides as Model.fold does. Pure Python: no library is loaded."""
import numpy as np
import pytest

import test_gpu_spanner_shapes as shapes
from test_gpu_spanner import INT64_MIN, Model

T = 1024  # gsamd.SPANNER_TILE (pinned to the kernels in test_spanner_capi.py)


def _plain(k, folds):
    model = Model(k)
    return [model.fold(s.tolist(), d.tolist()) for s, d in folds], model


@pytest.mark.parametrize("k", shapes.KS)
def test_fan_paths_put_the_boundary_at_k(k):
    """All 54 cases of k: every body edge is accepted, the closer iff L > k; INT64_MIN is a path
    endpoint with a fan; every route and round cap of the restatement gives the plain fold's mask."""
    st = shapes.fan_stream(k)
    cases = st["cases"]
    assert len(cases) == 54 and len({c["case"] for c in cases}) == 54
    assert {c["case"][0] for c in cases} == {k, k + 1} and {c["case"][1:] for c in cases} == {
        (a, b, c) for a in (0, 3, 70) for b in (0, 3, 70) for c in (0, 3, 70)}
    assert sum(c["s"] == INT64_MIN for c in cases) == 1
    (body, closers), model = _plain(k, shapes.fan_folds(k, "two")[0])
    assert all(body) and closers == [c["case"][0] > k for c in cases]
    cs, cd = st["closers"]
    for i, c in enumerate(cases):  # alternating orientation; s and t exactly L apart before the closer
        assert (int(cs[i]), int(cd[i])) == ((c["t"], c["s"]) if i % 2 else (c["s"], c["t"]))
    before = Model(k)
    before.fold(*(x.tolist() for x in st["body"]))
    for c in cases:
        L = c["case"][0]
        assert before.within(c["s"], c["t"], L) and not before.within(c["s"], c["t"], L - 1)
        assert (c["leaf"] is None) == (c["case"][1] == 0)
        if c["leaf"] is not None:
            assert before.within(c["leaf"], c["t"], L + 1) and not before.within(c["leaf"], c["t"], L)
    for route in ("two", "one", "mixed"):
        folds, owner = shapes.fan_folds(k, route)
        plain, plain_model = _plain(k, folds)
        assert sum(len(f[0]) for f in folds) == len(owner) == len(st["body"][0]) + 54
        for cap in (None, 0, shapes.HUGE) if route == "one" else (None,):
            mask, stats, model = shapes.fan_expect(k, route, cap)
            assert mask.tolist() == [m for f in plain for m in f], (route, cap)
            assert model.adj == plain_model.adj
            assert all(s["filter_drops"] + s["pending"] == len(f[0]) for s, f in zip(stats, folds))
    # the mixed route: every interior path vertex has an entry in either fold
    (es, ed), (os_, od) = shapes.fan_folds(k, "mixed")[0]
    first, second = set(es.tolist()) | set(ed.tolist()), set(os_.tolist()) | set(od.tolist())
    interior = sum(c["case"][0] - 1 for c in cases)
    assert len(first & second) >= interior


def test_fan_path_shape():
    body, (s, t), n, leaf = shapes.fan_path(5, 3, 70, 0)
    assert (s, t, n, leaf) == (0, 5, 6 + 73, 6) and len(body) == 5 + 73
    assert [e for e in body if e[1] == 5 and e[0] > 5] == [(v, 5) for v in range(9, 79)]
    body, _, n, leaf = shapes.fan_path(1, 0, 0, 3)  # the middle of one edge is s
    assert leaf is None and n == 5 and body[1:] == [(2, 0), (3, 0), (4, 0)]


@pytest.mark.parametrize("k,p", shapes.LADDERS)
def test_ladders_alternate_and_decide_one_rung_a_round(k, p):
    R = shapes.RUNGS
    for same_fold in (False, True):
        folds = shapes.ladder_folds(k, R, p, same_fold)
        plain, _ = _plain(k, folds)
        assert plain[-1][-R:] == [i % 2 == 0 for i in range(R)] and all(plain[0][:-R] if same_fold else plain[0])
        assert any(INT64_MIN in (s, d) for s, d in zip(*(x[-R:].tolist() for x in folds[-1])))  # a rung end
        for cap in (None, shapes.HUGE) if same_fold else (None, 0, 1, 3, shapes.HUGE):  # (as the GPU tests)
            mask, stats, _ = shapes.ladder_expect(k, R, p, same_fold, cap)
            assert mask.tolist() == [m for f in plain for m in f], (same_fold, cap)
            want = {None: 2 if same_fold else 1, shapes.HUGE: R}.get(cap, cap)
            assert (stats[-1]["rounds"], stats[-1]["tail"]) == (want, R - want if want else stats[-1]["pending"])
        assert shapes.ladder_expect(k, R, p, False, None)[1][-1]["pending"] == R


def test_twelve_rung_ladder_counts():
    """The rounds and tails of a 12-rung ladder, by hand: one rung a round, and under the product
    rule one of eleven or twelve is slow progress."""
    for k, p in shapes.LADDERS:
        got = {}
        for same_fold, caps in ((False, (None, 0, 1, 3, shapes.HUGE)), (True, (None, shapes.HUGE))):
            for cap in caps:
                st = shapes._expect(k, shapes.ladder_folds(k, 12, p, same_fold), cap)[1][-1]
                got[same_fold, cap] = (st["rounds"], st["tail"])
        assert got == {(False, None): (1, 11), (False, 0): (0, 12), (False, 1): (1, 11), (False, 3): (3, 9),
                       (False, shapes.HUGE): (12, 0), (True, None): (2, 10), (True, shapes.HUGE): (12, 0)}, (k, p)


def test_long_ladder():
    mask, stats, _ = shapes.ladder_expect(3, 300, 1, False, 0)
    assert mask[-300:].tolist() == [i % 2 == 0 for i in range(300)]
    assert stats[-1] == {"filter_drops": 0, "pending": 300, "rounds": 0, "tail": 300}


def test_slow_rule_argument():
    src, dst = shapes.ladder_folds(3, 12, 1, True)[0]
    want = Model(3).fold(src.tolist(), dst.tolist())
    for cap, slow, rounds in ((None, None, 2), (None, False, 12), (5, True, 2), (5, None, 5)):
        mask, r, tail, drops = Model(3).fold_rounds(src.tolist(), dst.tolist(), cap, slow)
        assert (mask, r, drops) == (want, rounds, 0) and tail == 12 - r, (cap, slow)


@pytest.mark.parametrize("a,b", shapes.HUBS)
def test_hub_streams(a, b):
    (fs, fd), (ss, sd) = shapes.hub_folds(a, b)
    hub = INT64_MIN
    assert (fs == hub).all() and len(set(fd.tolist())) == a
    old = set(fd.tolist())
    new = (set(ss.tolist()) | set(sd.tolist())) - old - {hub}
    assert len(new) == b
    pairs = list(zip(ss.tolist(), sd.tolist()))
    kinds = {"spoke": 0, "old-old": 0, "old-new": 0, "new-new": 0}
    spoke_at, early = {}, 0
    for i, (s, t) in enumerate(pairs):
        if hub in (s, t):
            kinds["spoke"] += 1
            spoke_at[t if s == hub else s] = i
    for i, (s, t) in enumerate(pairs):
        if hub in (s, t):
            continue
        kinds["old-old" if {s, t} <= old else "new-new" if {s, t} <= new else "old-new"] += 1
        early += any(x in new and spoke_at[x] > i for x in (s, t))
    assert kinds["spoke"] == b and min(kinds.values()) >= b // 5 and early >= b // 4
    for k in (1, 2):
        (first, second), _ = shapes.hub_expect(a, b, k)
        assert first.all() and second.any() and not second.all()
        if k == 1:  # an edge is dropped iff it arrived before (some new-new edges arrive twice)
            seen = set()
            fresh = [not (frozenset(e) in seen or seen.add(frozenset(e))) for e in pairs]
            assert second.tolist() == fresh and not all(fresh)
    # at k = 2 an arrival before its leaf's spoke is accepted and the spoke then dropped
    second = shapes.hub_expect(a, b, 2)[0][1]
    assert not all(second[i] for i in spoke_at.values())


def test_loop_stream():
    ids, src, dst = shapes.loop_stream()
    assert ids[0] == INT64_MIN and len(src) == 10 * 2 + 9 * 2
    loops = src == dst
    assert loops.sum() == 20 and all((src[loops] == v).sum() == 2 for v in ids)
    pairs = list(zip(src.tolist(), dst.tolist()))
    assert all((t, s) in pairs for s, t in pairs)
    for k in (1, 2):
        model = Model(k)
        mask = model.fold(src.tolist(), dst.tolist())
        assert sum(mask) == 19 and [m for m, l in zip(mask, loops) if l] == [True, False] * 10
        assert model.fold_rounds(src.tolist(), dst.tolist())[0] == [False] * len(src)
        assert Model(k).fold_rounds(src.tolist(), dst.tolist(), 0)[0] == mask


def test_tile_closed_form_is_the_models():
    n = T + 1
    src, dst = shapes.tile_pairs(n)
    assert src[0] == INT64_MIN and len(set(src.tolist()) | set(dst.tolist())) == 2 * n
    subsets = shapes.tile_subsets(n, T)
    assert {k: int(v.sum()) for k, v in subsets.items()} == {
        "none": 0, "all": n, "even": T // 2 + 1, "tile_last": 1, "tile_first": 2, "all_but_last": n - 1}
    for name, pre in subsets.items():
        want, stats, lo, hi = shapes.tile_expect(src, dst, pre)
        model = Model(3)
        for s, t in zip(src[pre].tolist(), dst[pre].tolist()):
            model.add(s, t)
        mask, rounds, tail, drops = model.fold_rounds(src.tolist(), dst.tolist())
        assert mask == want.tolist(), name
        assert {"filter_drops": drops, "pending": n - drops, "rounds": rounds, "tail": tail} == stats, name
        assert model.edges() == list(zip(lo.tolist(), hi.tolist())), name


def test_two_stars():
    ids, src, dst, la, lb = shapes.two_stars()
    assert ids[0] == INT64_MIN and len(src) == 17
    model = Model(3)
    assert all(model.fold(src.tolist(), dst.tolist()))
    assert model.within(la, lb, 3) and not model.within(la, lb, 2) and not model.within(lb, la, 2)
    assert len(model.adj[int(ids[0])]) == len(model.adj[int(ids[1])]) == 9


def test_restatement_on_random_streams():
    """Model.fold_rounds against Model.fold on random streams with repeats and loops, for the
    product rule and fixed caps."""
    rng = np.random.default_rng(7)
    for n, m, k in ((8, 30, 1), (12, 60, 2), (30, 80, 3), (40, 60, 5)):
        src, dst = rng.integers(0, n, m).tolist(), rng.integers(0, n, m).tolist()
        cut = m // 3
        for cap in (None, 0, 1, 2, shapes.HUGE):
            plain, rounds = Model(k), Model(k)
            want = plain.fold(src[:cut], dst[:cut]) + plain.fold(src[cut:], dst[cut:])
            got = [rounds.fold_rounds(src[:cut], dst[:cut], cap), rounds.fold_rounds(src[cut:], dst[cut:], cap)]
            assert got[0][0] + got[1][0] == want and rounds.adj == plain.adj, (n, m, k, cap)
            for mask, r, tail, drops in got:
                assert r <= (16 if cap is None else cap) and (tail == 0 or cap != shapes.HUGE)
                assert tail == len(mask) - drops if cap == 0 else tail <= len(mask) - drops
