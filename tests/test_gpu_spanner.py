"""GPU: the k-spanner summary (gs_spanner_*, gsamd.Spanner) against a restatement of
AdjacencyListGraph.boundedBFS and Spanner.UpdateLocal written from the contract in
include/gs_summary.h, the reference's own pins (tests/golden/spanner_pins.json), and the spanner
property checked on the export alone."""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MIN = -(1 << 63)


class Model:
    """AdjacencyListGraph + UpdateLocal, sequentially."""

    def __init__(self, k):
        self.k, self.adj = k, {}

    def within(self, s, t, k=None):
        if s not in self.adj:
            return False
        if s == t:
            return s in self.adj[s]
        seen, frontier = {s}, [s]
        for _ in range(self.k if k is None else k):
            nxt = []
            for u in frontier:
                for y in self.adj[u]:
                    if y == t:
                        return True
                    if y not in seen:
                        seen.add(y)
                        nxt.append(y)
            frontier = nxt
        return False

    def add(self, s, t):
        self.adj.setdefault(s, set()).add(t)
        self.adj.setdefault(t, set()).add(s)

    def fold(self, src, dst):
        out = []
        for s, t in zip(src, dst):
            out.append(not self.within(s, t))
            if out[-1]:
                self.add(s, t)
        return out

    def fold_rounds(self, src, dst, round_cap=None, slow_rule=None):
        """SpannerSeq::fold_rounds (csrc/gs_spanner_seq.hpp) as the device drives it: the filter
        pass on G0, rounds that read the statuses of the round before, then the tail in arrival
        order. round_cap None: the product rule (16 rounds, and -- slow_rule -- a round that
        decides less than 1/8 of its edges is the last); a set cap fixes the rounds alone.
        Returns (mask, rounds, tail, filter_drops); the graph ends as after fold()."""
        cap = 16 if round_cap is None else round_cap
        slow_rule = round_cap is None if slow_rule is None else slow_rule
        pend = [i for i, (s, t) in enumerate(zip(src, dst)) if not self.within(s, t)]
        st = [0] * len(pend)  # 0 undecided, 1 accepted, 2 dropped

        rows = {}  # vertex -> [(neighbour, pending index)]
        for j, a in enumerate(pend):
            rows.setdefault(src[a], []).append((dst[a], j))
            rows.setdefault(dst[a], []).append((src[a], j))

        def view(i, upper, status):  # within k in G0 + the pending j < i that are accepted / not dropped?
            s, t = src[pend[i]], dst[pend[i]]
            seen, frontier = {s}, [s]
            for _ in range(1 if s == t else self.k):  # (only its own loop reaches s again)
                nxt = []
                for u in frontier:
                    more = [y for y, j in rows.get(u, ()) if j < i and (status[j] == 1 or (upper and status[j] == 0))]
                    for y in (*self.adj.get(u, ()), *more):
                        if y == t:
                            return True
                        if y not in seen:
                            seen.add(y)
                            nxt.append(y)
                frontier = nxt
            return False

        rounds, und = 0, len(pend)
        while und and rounds < cap:
            nst = list(st)
            for i in range(len(pend)):
                if st[i] == 0:
                    nst[i] = 1 if not view(i, True, st) else 2 if view(i, False, st) else 0
            before, st, und = und, nst, nst.count(0)
            rounds += 1
            if slow_rule and (before - und) * 8 < before:
                break
        tail = und
        for i in range(len(pend)):
            if st[i] == 0:
                st[i] = 2 if view(i, False, st) else 1
        mask = [False] * len(src)
        for i, j in enumerate(pend):
            if st[i] == 1:
                mask[j] = True
                self.add(src[j], dst[j])
        return mask, rounds, tail, len(src) - len(pend)

    def edges(self):
        return sorted((u, v) for u in self.adj for v in self.adj[u] if u <= v)


def _pins():
    with open(os.path.join(ROOT, "tests", "golden", "spanner_pins.json")) as f:
        return json.load(f)


def _scramble(v, salt):
    """Dense ids 0.. to sparse signed 64-bit ids, negatives among them."""
    x = (v.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(salt * 0x632BE5AB + 1)
    x ^= x >> np.uint64(29)
    return x.view(np.int64)


SIZES = [(n, m) for n in (8, 40, 200) for m in (10, 60, 400)]
KS = (1, 2, 3, 5)


@functools.lru_cache(maxsize=None)
def _stream(n, m, k, min_id=False):
    """(src, dst, accepted mask, edges) of a random stream over n vertices, with repeats and loops."""
    rng = np.random.default_rng(1000 * n + 10 * m + k)
    with np.errstate(over="ignore"):
        ids = _scramble(np.arange(n), n + m)
    if min_id:
        ids[0] = INT64_MIN
    assert len(set(ids.tolist())) == n and (ids < 0).any()
    src = ids[rng.integers(0, n, m)]
    dst = ids[rng.integers(0, n, m)]
    model = Model(k)
    mask = np.array(model.fold(src.tolist(), dst.tolist()), dtype=bool)
    return src, dst, mask, model.edges()


def _edges_of(sp):
    lo, hi = sp.edges()
    return list(zip(lo.tolist(), hi.tolist()))


def _run(gs, src, dst, k, batch):
    """Fold the stream in batches; returns (mask, edges, count, the folds' stats)."""
    stats = []
    with gs.Spanner(k=k, edge_hint=16) as sp:
        mask = []
        for i in range(0, len(src), batch):
            mask.append(sp.fold(src[i:i + batch], dst[i:i + batch]))
            stats.append(sp.stats())
        return np.concatenate(mask), _edges_of(sp), sp.count(), stats


def test_pinned_within_sequence(gs):
    pin = _pins()["bounded_bfs"]
    with gs.Spanner(k=pin["k"]) as sp:
        e = np.array(pin["initial_edges"], dtype=np.int64)
        assert sp.fold(e[:, 0], e[:, 1]).all()
        got = []
        for step in pin["steps"]:
            s, t = step["query"]
            got.append(bool(sp.within([s], [t], pin["k"])[0]))
            assert bool(sp.fold([s], [t])[0]) == step["add"]
        assert got == [False, False, True, False, False, True] == [s["within"] for s in pin["steps"]]


def test_pinned_add_edge_sequence(gs):
    pin = _pins()["add_edge"]
    with gs.Spanner(k=3) as sp:
        for step in pin["steps"]:
            sp.add([step["edge"][0]], [step["edge"][1]])
            v, off, nb = sp.neighbors()
            rows = {str(x): nb[off[i]:off[i + 1]].tolist() for i, x in enumerate(v.tolist())}
            assert rows == step["rows"]
            assert sp.count()[1] == step["vertices_after"] == len(v)


def test_add_is_unconditional(gs):
    """addEdge does not ask the spanner's k: every edge of the stream is in the graph afterwards."""
    src, dst, _, _ = _stream(40, 60, 3)
    with gs.Spanner(k=3) as sp:
        sp.add(src[:25], dst[:25])
        sp.add(src[25:], dst[25:])
        want = sorted({(min(s, t), max(s, t)) for s, t in zip(src.tolist(), dst.tolist())})
        assert _edges_of(sp) == want and sp.count()[0] == len(want)
        assert sp.within(src, dst, 1).all()


@pytest.mark.parametrize("batch", [12, 1, 5])
def test_default_stream(gs, batch):
    pin = _pins()["default_stream"]
    e = np.array(pin["edges"], dtype=np.int64)
    mask, edges, count, _ = _run(gs, e[:, 0], e[:, 1], pin["k"], batch)
    assert np.flatnonzero(mask).tolist() == pin["accepted_arrivals"]
    assert [pin["edges"][i] for i in np.flatnonzero(~mask)] == pin["dropped_edges"]
    assert edges == sorted((min(a, b), max(a, b)) for a, b in e[mask].tolist())
    assert count == (9, 9)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,m", SIZES)
def test_random_streams_match_the_restatement(gs, n, m, k):
    src, dst, want, want_edges = _stream(n, m, k)
    for batch in (1, 7, m):
        mask, edges, count, _ = _run(gs, src, dst, k, batch)
        assert np.array_equal(mask, want), (batch, np.flatnonzero(mask != want)[:8])
        assert edges == want_edges, batch
        assert count == (len(want_edges), len({x for e in want_edges for x in e}))


def test_int64_min_is_a_vertex_like_any_other(gs):
    src, dst, want, want_edges = _stream(40, 60, 3, True)
    assert (src == INT64_MIN).any() or (dst == INT64_MIN).any()
    for batch in (1, 7, 60):
        mask, edges, _, _ = _run(gs, src, dst, 3, batch)
        assert np.array_equal(mask, want) and edges == want_edges, batch
    with gs.testing(spanner_lds_set=4):
        mask, edges, _, _ = _run(gs, src, dst, 3, 60)
        assert np.array_equal(mask, want) and edges == want_edges


def _whole_stream_cases(gs):
    out = []
    for n, m in SIZES:
        for k in KS:
            src, dst, want, want_edges = _stream(n, m, k)
            mask, edges, _, stats = _run(gs, src, dst, k, m)
            assert np.array_equal(mask, want) and edges == want_edges, (n, m, k)
            out.append(stats[0])
    return out


def test_rounds_are_used(gs):
    stats = _whole_stream_cases(gs)
    assert max(s["rounds"] for s in stats) >= 3
    for s in stats:
        assert s["filter_drops"] + s["pending"] in (10, 60, 400)


def test_round_cap_one_leaves_the_rest_to_the_tail(gs):
    with gs.testing(spanner_round_cap=1):
        stats = _whole_stream_cases(gs)
    assert all(s["rounds"] <= 1 for s in stats)
    assert max(s["tail"] for s in stats) > 0


def test_round_cap_huge_leaves_no_tail(gs):
    with gs.testing(spanner_round_cap=1 << 40):
        stats = _whole_stream_cases(gs)
    assert all(s["tail"] == 0 for s in stats)
    assert max(s["rounds"] for s in stats) >= 3


def test_round_cap_zero_is_all_tail(gs):
    with gs.testing(spanner_round_cap=0):
        stats = _whole_stream_cases(gs)
    assert all(s["rounds"] == 0 and s["tail"] == s["pending"] for s in stats)


@pytest.mark.parametrize("arenas", [None, 1])
def test_tiny_on_chip_sets_force_the_heavy_path(gs, arenas):
    with gs.testing(spanner_lds_set=4, spanner_arenas=arenas):
        stats = _whole_stream_cases(gs)
        assert sum(s["heavy"] for s in stats) > 0
        for n, m, k in ((40, 60, 3), (200, 400, 2)):  # in small folds too
            src, dst, want, want_edges = _stream(n, m, k)
            mask, edges, _, _ = _run(gs, src, dst, k, 7)
            assert np.array_equal(mask, want) and edges == want_edges


@pytest.mark.parametrize("arenas", [None, 1])
def test_star_overflows_the_product_sets(gs, arenas):
    """Two stars of more leaves than the on-chip sets hold. Leaf to leaf inside a star is two edges:
    dropped. Leaf to leaf across the stars has no path: the search must finish the whole ball of
    a star, which the heavy path does, exactly."""
    leaves = gs.SPANNER_LDS_SET + 44
    a = np.arange(1, leaves + 1, dtype=np.int64) * 7 - 5000
    b = np.arange(1, leaves + 1, dtype=np.int64) * 11 + (1 << 40)
    ca, cb = np.int64(-3), np.int64(1 << 50)
    with gs.testing(spanner_arenas=arenas), gs.Spanner(k=3) as sp:
        model = Model(3)
        star_s = np.concatenate([np.full(leaves, ca), np.full(leaves, cb)])
        star_d = np.concatenate([a, b])
        assert sp.fold(star_s, star_d).all()
        model.fold(star_s.tolist(), star_d.tolist())
        inside = sp.fold(a[:-1], a[1:])
        assert not inside.any() and sp.count() == (2 * leaves, 2 * leaves + 2)
        cross_s = np.concatenate([a[:20], a[:20]])
        cross_d = np.concatenate([b[:20], b[20:0:-1]])
        got = sp.fold(cross_s, cross_d)
        assert sp.stats()["heavy"] > 0 and sp.stats()["longest_row"] >= leaves
        assert got.tolist() == model.fold(cross_s.tolist(), cross_d.tolist())
        assert got[0] and not got.all()
        assert _edges_of(sp) == model.edges()
        # a ball that is the whole graph: every k up to the limit, from a leaf nothing reaches
        far = np.int64(INT64_MIN)
        sp.fold([far], [far + 1])
        for k in (4, 16):
            assert sp.within([a[30], a[30], a[30]], [far, b[30], a[31]], k).tolist() == [
                model.within(int(a[30]), int(far), k), model.within(int(a[30]), int(b[30]), k), True]


def test_in_batch_dependence(gs):
    with gs.Spanner(k=3) as sp:
        same = sp.fold(np.full(1000, 17), np.full(1000, -4))
        assert same.tolist() == [True] + [False] * 999
        st = sp.stats()  # round 1 accepts the first, which is slow progress: the tail drops the rest
        assert st["filter_drops"] == 0 and st["pending"] == 1000 and st["rounds"] == 1 and st["tail"] == 999
        sp.reset()
        with gs.testing(spanner_round_cap=1 << 40):  # rounds alone: the second one drops the rest
            assert sp.fold(np.full(1000, 17), np.full(1000, -4)).tolist() == [True] + [False] * 999
            assert sp.stats()["rounds"] == 2 and sp.stats()["tail"] == 0
        sp.reset()
        path = np.arange(2001, dtype=np.int64) * 3 - 3000
        assert sp.fold(path[:-1], path[1:]).all() and sp.count() == (2000, 2001)
        sp.reset()
        assert sp.fold([5, 5], [5, 5]).tolist() == [True, False]
        assert sp.fold([5], [5]).tolist() == [False]
        assert sp.count() == (1, 1) and _edges_of(sp) == [(5, 5)]
        v, off, nb = sp.neighbors()
        assert v.tolist() == [5] and off.tolist() == [0, 1] and nb.tolist() == [5]
        assert sp.within([5, 5, 6], [5, 6, 6], 3).tolist() == [True, False, False]


@pytest.mark.parametrize("k", KS)
def test_spanner_property_on_the_export_alone(gs, k):
    src, dst, _, _ = _stream(200, 400, k)
    _, edges, _, _ = _run(gs, src, dst, k, 64)
    streamed = {(min(s, t), max(s, t)) for s, t in zip(src.tolist(), dst.tolist())}
    assert set(edges) <= streamed and len(set(edges)) == len(edges)
    adj = {}
    for u, v in edges:
        adj.setdefault(u, set()).add(v)
        adj.setdefault(v, set()).add(u)
    for s, t in streamed:
        if s == t:
            continue
        seen, frontier, dist = {s}, [s], 0
        while t not in seen and frontier and dist < k:
            frontier = [y for u in frontier for y in adj.get(u, ()) if y not in seen and not seen.add(y)]
            dist += 1
        assert t in seen, (s, t)


def test_combine_folds_the_other_export_in_ascending_order(gs):
    src, dst, _, _ = _stream(200, 400, 3)
    with gs.Spanner(k=3) as a, gs.Spanner(k=2) as b:
        a.fold(src[:200], dst[:200])
        b.fold(src[200:], dst[200:])
        model = Model(3)
        model.fold(src[:200].tolist(), dst[:200].tolist())
        b_edges = _edges_of(b)
        assert b_edges == sorted(b_edges) and _edges_of(a) == model.edges()
        model.fold([e[0] for e in b_edges], [e[1] for e in b_edges])
        a.combine(b)
        assert _edges_of(a) == model.edges()
        assert _edges_of(b) == b_edges and b.count()[0] == len(b_edges)
        n_before = a.count()
        a.combine(a)  # every edge is within 1 of itself
        assert a.count() == n_before


def test_reset_gives_an_empty_graph_that_folds_again(gs):
    src, dst, want, want_edges = _stream(40, 60, 2)
    with gs.Spanner(k=2) as sp:
        sp.fold(src[::-1], dst[::-1])
        sp.reset()
        assert sp.count() == (0, 0) and _edges_of(sp) == [] and sp.neighbors()[0].size == 0
        assert not sp.within(src[:4], dst[:4]).any()
        assert np.array_equal(sp.fold(src, dst), want) and _edges_of(sp) == want_edges


def test_device_variants(gs):
    import torch
    src, dst, want, want_edges = _stream(200, 400, 3)
    dev = torch.device("cuda:0")
    ts, td = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    inter = torch.stack([ts, td], dim=1).contiguous().view(-1)  # stride 2
    acc = torch.zeros(400, dtype=torch.uint8, device=dev)
    with gs.Spanner(k=3) as sp:
        torch.cuda.synchronize()
        sp.fold_device(inter, inter[1:], acc, n=400, stride=2)
        sp.sync()
        assert np.array_equal(acc.cpu().numpy().astype(bool), want)
        lo = torch.empty(len(want_edges), dtype=torch.int64, device=dev)
        hi = torch.empty_like(lo)
        assert sp.edges_device(lo, hi) == len(want_edges)
        assert list(zip(lo.cpu().tolist(), hi.cpu().tolist())) == want_edges
        with pytest.raises(gs.GSError) as e:
            sp.edges_device(lo[:1], hi[:1])
        assert e.value.code == gs.GS_ERR_TRUNCATED
        out = torch.zeros(400, dtype=torch.uint8, device=dev)
        sp.within_device(ts, td, out)
        sp.sync()
        assert out.cpu().numpy().all()  # every streamed edge with distinct ends is spanned; loops were kept
