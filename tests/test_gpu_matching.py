"""GPU: the weighted matching summary (gs_matching_*, gsamd.Matching) against a restatement of
CentralizedWeightedMatching's flatMap written from the contract in include/gs_summary.h: the
accepted bytes, the event rows and the exported M, under every tuning of the round scheme, and
the hand-worked pins of tests/golden/matching_pins.json."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
ADD, REMOVE = 0, 1


def _wrap(x):
    """Java long arithmetic."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


class Model:
    """M kept per vertex: at[v] = (src, dst, value, global arrival number of the acceptance)."""

    def __init__(self):
        self.at, self.folded = {}, 0

    def fold(self, src, dst, val):
        """(accepted list, event rows (arrival, type, src, dst, val)) of one fold."""
        acc, ev = [], []
        for i, (u, v, w) in enumerate(zip(src, dst, val)):
            hits = []  # the edge at the source endpoint first, then the one at the target endpoint
            for x in (u, v):
                if x in self.at and self.at[x] not in hits:
                    hits.append(self.at[x])
            ok = w > _wrap(2 * _wrap(sum(e[2] for e in hits)))
            acc.append(ok)
            if ok:
                for e in hits:
                    ev.append((i, REMOVE, e[0], e[1], e[2]))
                    self.at.pop(e[0])
                    self.at.pop(e[1], None)
                self.at[u] = self.at[v] = (u, v, w, self.folded)
                ev.append((i, ADD, u, v, w))
            self.folded += 1
        return acc, ev

    def edges(self):
        return sorted(set(self.at.values()), key=lambda e: e[3])

    def weight(self):
        return _wrap(sum(e[2] for e in self.edges()))


def _events_of(m):
    a, t, s, d, w = m.events()
    return list(zip(a.tolist(), t.tolist(), s.tolist(), d.tolist(), w.tolist()))


def _edges_of(m):
    s, d, w, f = m.edges()
    return list(zip(s.tolist(), d.tolist(), w.tolist(), f.tolist()))


def _check(gs, src, dst, val, cuts=None, tune=None, hint=16):
    """Fold the stream (whole, or cut at `cuts`) and compare everything with the model; returns the
    stats of every fold and the handle's final stats."""
    src, dst, val = (np.asarray(x, dtype=np.int64) for x in (src, dst, val))
    bounds = [0] + sorted(cuts or []) + [len(src)]
    model = Model()
    stats = []
    with gs.Matching(vertex_hint=hint) as m:
        if tune:
            m.tune(**tune)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            want_acc, want_ev = model.fold(src[lo:hi].tolist(), dst[lo:hi].tolist(), val[lo:hi].tolist())
            acc = m.fold(src[lo:hi], dst[lo:hi], val[lo:hi])
            assert acc.tolist() == want_acc
            assert _events_of(m) == want_ev
            stats.append(m.stats())
            assert stats[-1]["accepted"] == sum(want_acc)
        assert _edges_of(m) == model.edges()
        e, nv, weight = m.count()
        assert e == len(model.edges()) and weight == model.weight()
        assert nv == len(set(src.tolist()) | set(dst.tolist()))
    return stats


def _scramble(v, salt):
    """Dense ids 0.. to sparse signed 64-bit ids, negatives among them."""
    with np.errstate(over="ignore"):
        x = (v.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(salt * 0x632BE5AB + 1)
    x ^= x >> np.uint64(29)
    return x.view(np.int64)


MODES = ("unit", "small", "pow2", "uniform")


@functools.lru_cache(maxsize=None)
def _stream(nv, n, mode, seed=0):
    rng = np.random.default_rng(97 * nv + 13 * n + 7 * MODES.index(mode) + seed)
    ids = _scramble(np.arange(nv), nv + n)
    src = ids[rng.integers(0, nv, n)]
    dst = ids[rng.integers(0, nv, n)]
    if mode == "unit":
        val = np.ones(n, np.int64)
    elif mode == "small":
        val = rng.integers(10, 51, n)
    elif mode == "pow2":
        val = np.int64(1) << rng.integers(0, 40, n)
    else:
        val = rng.integers(0, 1 << 50, n)
    return src, dst, val.astype(np.int64)


def _cuts(n, seed):
    """Random cut points, an empty and a one-edge fold among them."""
    rng = np.random.default_rng(seed)
    c = sorted(rng.integers(0, n + 1, 6).tolist())
    return sorted(c + [c[2], min(c[4] + 1, n)])


def _pins():
    with open(os.path.join(ROOT, "tests", "golden", "matching_pins.json")) as f:
        return json.load(f)["streams"]


@pytest.mark.parametrize("name", ["doubling_star", "unit_path", "bridge"])
def test_pinned_streams(gs, name):
    pin = _pins()[name]
    e = np.array(pin["edges"], dtype=np.int64)
    with gs.Matching(vertex_hint=0) as m:
        acc = m.fold(e[:, 0], e[:, 1], e[:, 2])
        assert np.flatnonzero(acc).tolist() == pin["accepted_arrivals"]
        assert _events_of(m) == [tuple(r) for r in pin["events"]]
        assert _edges_of(m) == [tuple(r) for r in pin["matching"]]
        assert m.count() == (len(pin["matching"]), len(set(e[:, :2].ravel().tolist())), pin["weight"])
    _check(gs, e[:, 0], e[:, 1], e[:, 2])


def test_empty_fold_one_edge_loops_and_repeats(gs):
    with gs.Matching() as m:
        assert m.fold([], [], []).tolist() == []
        assert _events_of(m) == [] and _edges_of(m) == [] and m.count() == (0, 0, 0)
        assert m.fold([5], [9], [3]).tolist() == [True]
        assert _events_of(m) == [(0, ADD, 5, 9, 3)]
        assert m.fold([], [], []).tolist() == [] and _events_of(m) == []
        assert _edges_of(m) == [(5, 9, 3, 0)]
    # loops (a loop is its vertex's edge), repeats (w > 2 w is false), reversed repeats, non-positive values
    src = [1, 1, 1, 2, 2, 1, 3, 3, 2, 4, 4, 4, 1]
    dst = [1, 1, 2, 1, 2, 1, 3, 3, 3, 4, 5, 4, 2]
    val = [4, 4, 9, 9, 19, 50, 0, -5, 7, 1, 3, 7, 9]
    _check(gs, src, dst, val)
    _check(gs, src, dst, val, cuts=[1, 2, 2, 7])


def test_extreme_negative_and_sparse_ids(gs):
    ids = [INT64_MIN, INT64_MAX, -1, 0, 1, INT64_MIN + 1, INT64_MAX - 1, -(1 << 40), 1 << 40, 12345678901234]
    rng = np.random.default_rng(5)
    src = [ids[i] for i in rng.integers(0, len(ids), 80)]
    dst = [ids[i] for i in rng.integers(0, len(ids), 80)]
    val = rng.integers(1, 100, 80).tolist()
    _check(gs, src, dst, val, hint=0)
    _check(gs, src, dst, val, cuts=[3, 40, 41])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nv,n", [(2, 50), (8, 300), (64, 2000), (1024, 4096)])
def test_random_streams_whole_and_cut(gs, nv, n, mode):
    src, dst, val = _stream(nv, n, mode)
    _check(gs, src, dst, val)
    _check(gs, src, dst, val, cuts=_cuts(n, nv + n))


DOORS = {"product": {}, "all_tail": {"round_cap": 0}, "no_tail": {"round_cap": 1 << 40}, "one_pass": {"iter_cap": 1},
         "one_pass_no_tail": {"iter_cap": 1, "round_cap": 1 << 40}, "unsharpened": {"sharpen": False},
         "unsharpened_no_tail": {"sharpen": False, "round_cap": 1 << 40}}


@pytest.mark.parametrize("door", sorted(DOORS))
@pytest.mark.parametrize("mode", ("unit", "small", "uniform"))
def test_every_door_gives_the_same_result(gs, door, mode):
    src, dst, val = _stream(300, 4096, mode, seed=3)
    n = len(src)
    stats = _check(gs, src, dst, val, tune=DOORS[door])[0]
    if "round_cap" not in DOORS[door]:
        return
    if DOORS[door]["round_cap"] == 0:
        assert stats["tail"] == n  # every arrival was pending when the tail took over
    else:
        assert stats["tail"] == 0 and stats["rounds"] >= 1
    if DOORS[door].get("iter_cap") == 1 and mode != "unit":
        assert stats["fallbacks"] >= 1


def test_product_rounds_above_the_tail_threshold(gs):
    n = 3 * gs.MATCHING_TAIL_THRESHOLD
    src, dst, val = _stream(5000, n, "small", seed=9)
    stats = _check(gs, src, dst, val)[0]
    assert 0 < stats["tail"] < gs.MATCHING_TAIL_THRESHOLD and stats["rounds"] >= 2


def test_wrapping_values_turn_weight_safety_off_until_reset(gs):
    rng = np.random.default_rng(11)
    pool = [1 << 62, INT64_MAX, INT64_MIN, -1, -7, (1 << 62) + 5, 3, 1, 0, 1 << 61, (1 << 61) - 1]
    n = 600
    src = rng.integers(0, 40, n)
    dst = rng.integers(0, 40, n)
    val = np.array([pool[i] for i in rng.integers(0, len(pool), n)], dtype=np.int64)
    for tune in ({}, {"round_cap": 1 << 40}, {"round_cap": 0}):
        _check(gs, src, dst, val, tune=tune)
        _check(gs, src, dst, val, cuts=_cuts(n, 3), tune=tune)
    with gs.Matching() as m:
        m.fold([1, 2], [2, 3], [5, (1 << 61) - 1])
        assert m.stats()["weight_safe"]
        m.fold([7], [8], [1 << 61])
        assert not m.stats()["weight_safe"]
        m.fold([9], [10], [1])
        assert not m.stats()["weight_safe"]
        m.reset()
        assert m.stats()["weight_safe"] and m.count() == (0, 0, 0) and _edges_of(m) == []
        assert m.fold([9], [10], [-1]).tolist() == [False]
        assert not m.stats()["weight_safe"]


def test_unit_path_in_path_order_is_a_chain_of_rounds(gs):
    v = np.arange(301, dtype=np.int64)
    for tune in ({}, {"round_cap": 1 << 40}):
        stats = _check(gs, v[:-1], v[1:], np.ones(300, np.int64), tune=tune)[0]
        assert stats["accepted"] == 150 and stats["rounds"] >= 100


def test_doubling_star_is_an_accept_chain_on_one_vertex(gs):
    leaves = np.arange(1, 41, dtype=np.int64)
    val = (np.int64(1) << leaves) - 1  # 1, 3, 7, ...: each more than twice the one before
    for tune in ({}, {"round_cap": 1 << 40}, {"sharpen": False}):
        stats = _check(gs, np.zeros(40, np.int64), leaves, val, tune=tune)[0]
        assert stats["accepted"] == 40


def test_hub_stream(gs):
    rng = np.random.default_rng(21)
    n = 2000
    src = rng.integers(1, 500, n)
    src[rng.random(n) < 0.6] = 0  # 60 % of the edges share vertex 0
    dst = rng.integers(1, 500, n)
    val = rng.integers(1, 1000, n)
    for tune in ({}, {"round_cap": 1 << 40}):
        _check(gs, src, dst, val, tune=tune)


def test_growth_from_no_hint(gs):
    rng = np.random.default_rng(31)
    a = np.arange(5000, dtype=np.int64) * 7 - 9000
    b = np.arange(5000, 9000, dtype=np.int64) * 7 - 9000
    src = np.concatenate([a[::2], b[::2], rng.choice(a, 500)])
    dst = np.concatenate([a[1::2], b[1::2], rng.choice(b, 500)])
    val = rng.integers(1, 50, len(src))
    _check(gs, src, dst, val, cuts=[2500, 4500], hint=0)


def test_device_inputs_with_stride_behind_a_producer_stream(gs):
    import torch
    src, dst, val = _stream(64, 2000, "small", seed=5)
    want_acc, want_ev = Model().fold(src.tolist(), dst.tolist(), val.tolist())
    dev = torch.device("cuda:0")
    producer = torch.cuda.Stream(device=dev)
    with gs.Matching() as m:
        with torch.cuda.stream(producer):
            inter = [torch.empty(2 * len(src), dtype=torch.int64, device=dev) for _ in range(3)]
            for t, x in zip(inter, (src, dst, val)):
                t.fill_(-77)
                t[::2] = torch.from_numpy(x).to(dev, non_blocking=True)
        acc = torch.zeros(len(src), dtype=torch.uint8, device=dev)
        m.fold_device(inter[0], inter[1], inter[2], accepted=acc, stride=2, after=producer)
        assert m.stream
        m.sync()
        assert acc.cpu().numpy().astype(bool).tolist() == want_acc
        rows = len(want_ev)
        out = [torch.zeros(rows, dtype=dt, device=dev) for dt in (torch.int32, torch.uint8, torch.int64, torch.int64,
                                                                   torch.int64)]
        assert m.events_device(*out) == rows
        m.sync()
        got = list(zip(*(t.cpu().numpy().tolist() for t in out)))
        assert got == want_ev
        e = m.count()[0]
        xs = [torch.zeros(e, dtype=torch.int64, device=dev) for _ in range(4)]
        assert m.edges_device(*xs) == e
        m.sync()
        assert list(zip(*(t.cpu().numpy().tolist() for t in xs))) == _edges_of(m)


def test_event_capacity_one_short_is_truncated_and_writes_nothing(gs):
    L = gs.lib()
    with gs.Matching() as m:
        m.fold([1, 3, 2], [2, 4, 3], [5, 5, 21])
        rows = 5
        a = np.full(rows, 99, np.uint32)
        t = np.full(rows, 99, np.uint8)
        s, d, w = (np.full(rows, 99, np.int64) for _ in range(3))
        n = ctypes.c_size_t(0)
        rc = L.gs_matching_events(m.handle, a.ctypes.data, t.ctypes.data, s.ctypes.data, d.ctypes.data, w.ctypes.data,
                                  rows - 1, ctypes.byref(n))
        assert rc == gs.GS_ERR_TRUNCATED and n.value == rows
        assert all((x == 99).all() for x in (a, t, s, d, w))
        n = ctypes.c_size_t(0)
        rc = L.gs_matching_export(m.handle, s.ctypes.data, d.ctypes.data, w.ctypes.data, None, 0, ctypes.byref(n))
        assert rc == gs.GS_ERR_TRUNCATED and n.value == 1 and (s == 99).all()
        rc = L.gs_matching_events(m.handle, a.ctypes.data, t.ctypes.data, s.ctypes.data, d.ctypes.data, w.ctypes.data,
                                  rows, ctypes.byref(n))
        assert rc == gs.GS_OK and n.value == rows and t.tolist() == [ADD, ADD, REMOVE, REMOVE, ADD]


def test_mate_device_on_present_and_absent_ids(gs):
    import torch
    dev = torch.device("cuda:0")
    with gs.Matching() as m:
        m.fold([1, 3, 2, 8, INT64_MIN], [2, 4, 3, 8, 6], [5, 5, 21, 2, 9])
        # M = (2, 3, 21), the loop (8, 8, 2), (INT64_MIN, 6, 9); 1 and 4 were seen and are unmatched
        q = torch.tensor([2, 3, 1, 4, 8, INT64_MIN, 6, 777, INT64_MAX], dtype=torch.int64, device=dev)
        mate = torch.full((9,), -5, dtype=torch.int64, device=dev)
        val = torch.full((9,), -5, dtype=torch.int64, device=dev)
        found = torch.full((9,), 7, dtype=torch.uint8, device=dev)
        m.mate_device(q, mate, val, found)
        m.sync()
        assert found.cpu().tolist() == [1, 1, 0, 0, 1, 1, 1, 0, 0]
        assert mate.cpu().tolist() == [3, 2, 0, 0, 8, 6, INT64_MIN, 0, 0]
        assert val.cpu().tolist() == [21, 21, 0, 0, 2, 9, 9, 0, 0]


def test_count_weight_against_the_export(gs):
    src, dst, val = _stream(64, 2000, "uniform", seed=8)
    with gs.Matching() as m:
        for lo in range(0, 2000, 500):
            m.fold(src[lo:lo + 500], dst[lo:lo + 500], val[lo:lo + 500])
            s, d, w, f = m.edges()
            e, nv, weight = m.count()
            assert e == len(s) and weight == _wrap(int(w.astype(object).sum()))
            # M is a matching: no vertex twice (a loop has one endpoint)
            assert (np.diff(f.astype(np.int64)) > 0).all()
            assert len(set(s.tolist()) | set(d.tolist())) == 2 * e - int((s == d).sum())


def test_hbm_bytes_return_after_close(gs):
    before = gs.hbm_bytes(0)
    src, dst, val = _stream(1024, 4096, "small")
    m = gs.Matching(vertex_hint=0)
    assert gs.hbm_bytes(0) > before
    m.fold(src, dst, val)
    m.events()
    m.edges()
    held = gs.hbm_bytes(0)
    assert held > before
    m.close()
    assert gs.hbm_bytes(0) == before
