"""GPU: the distinct streams (gsamd.Distinct, the gs_distinct_* calls) against a plain dict / set
restatement of the contract: an edge is new when its key is not in the set of keys seen so far
(the ordered pair in directed mode, the unordered pair in undirected mode), an endpoint entry is
new when its id is not in the set of ids seen so far; the first occurrence in arrival order is
the one kept. Everything is an integer: every comparison is exact. The reference's pinned
outputs (tests/golden/distinct_pins.json) are section 1. The shape cases sit at the tile of the
compaction kernels (T = gsamd.DISTINCT_TILE) and at a wave (64); stats() proves that a case
really crossed tiles, grew its tables and probed past a home slot."""
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
T = gsamd.DISTINCT_TILE
MODES = ("directed", "undirected")


class Truth:
    """first-seen = key not in set"""

    def __init__(self, mode):
        self.mode = mode
        self.ids, self.keys = set(), set()
        self.vlist, self.esrc, self.edst, self.efirst = [], [], [], []
        self.folded = 0

    def fold(self, src, dst):
        """((new vertex ids, their entries), (kept indices, src, dst)) of this fold."""
        nv, ne, idx = [], [], []
        for i, (s, d) in enumerate(zip(np.asarray(src, np.int64).tolist(), np.asarray(dst, np.int64).tolist())):
            for e, x in ((2 * i, s), (2 * i + 1, d)):
                if x not in self.ids:
                    self.ids.add(x)
                    self.vlist.append(x)
                    nv.append(x)
                    ne.append(e)
            key = (s, d) if self.mode == "directed" or s <= d else (d, s)
            if key not in self.keys:
                self.keys.add(key)
                idx.append(i)
                self.esrc.append(s)
                self.edst.append(d)
                self.efirst.append(self.folded + i)
        self.folded += len(src)
        return (nv, ne), idx


def _fold_and_check(ds, tr, src, dst):
    """One host fold compared with the truth, emissions included; returns the kept indices."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    (nv, nent), idx = tr.fold(src, dst)
    got = ds.fold(src, dst)
    assert got == (len(nv), len(idx))
    v, ent = ds.new_vertices()
    assert v.dtype == np.int64 and ent.dtype == np.uint32
    assert v.tolist() == nv and ent.tolist() == nent
    gi, gs_, gd = ds.new_edges()
    assert gi.dtype == np.uint32 and gi.tolist() == idx
    assert np.array_equal(gs_, src[idx]) and np.array_equal(gd, dst[idx])  # the orientation they arrived with
    assert ds.size() == (len(tr.vlist), len(tr.esrc), tr.folded, len(nv), len(idx))
    return idx


def _check_state(ds, tr):
    assert ds.vertices().tolist() == tr.vlist
    s, d, f = ds.edges()
    assert f.dtype == np.uint64
    assert s.tolist() == tr.esrc and d.tolist() == tr.edst and f.tolist() == tr.efirst


def _pins():
    with open(os.path.join(GOLD, "distinct_pins.json")) as f:
        return json.load(f)


# ---- 1. the reference's pinned outputs
def test_pins_distinct(gs):
    pins = _pins()
    e = np.array(pins["edges"]["rows"] * pins["distinct"]["input_repeats"], np.int64)
    with gs.Distinct() as ds:
        assert ds.fold(e[:, 0], e[:, 1]) == (5, 7)
        idx, s, d = ds.new_edges()
        rows = [list(r) for r in zip(s.tolist(), d.tolist(), e[idx, 2].tolist())]  # values through index
        assert rows == pins["distinct"]["rows"]
        assert idx.tolist() == list(range(7))
        # the literal mapper would have kept five
        assert len(pins["literal_mapper"]["kept_at_parallelism_one"]) == 5 != len(rows)


def test_pins_vertices_and_running_count(gs):
    pins = _pins()
    e = np.array(pins["edges"]["rows"], np.int64)
    with gs.Distinct() as ds:
        ds.fold(e[:, 0], e[:, 1])
        v, ent = ds.new_vertices()
        assert v.tolist() == pins["vertices"]["rows"] == ds.vertices().tolist()
        assert ent.tolist() == pins["vertices"]["entries"]
        # numberOfVertices emits rank + 1 at the entry of every new vertex
        import torch
        rank = torch.empty(len(v), dtype=torch.int64, device="cuda:0")
        dv = torch.from_numpy(v).to("cuda:0")
        ds.wait_stream("torch")
        ds.rank_device(dv, rank)
        ds.sync()
        assert (rank.cpu() + 1).tolist() == pins["number_of_vertices"]["rows"]
        assert list(range(1, ds.size()[2] + 1)) == pins["number_of_edges"]["rows"]


# ---- 2. smallest shapes
@pytest.mark.parametrize("mode", MODES)
def test_smallest_shapes(gs, mode):
    with gs.Distinct(mode=mode) as ds:
        tr = Truth(mode)
        _fold_and_check(ds, tr, [], [])
        assert ds.size() == (0, 0, 0, 0, 0)
        _check_state(ds, tr)
        _fold_and_check(ds, tr, [5], [9])  # one edge
        assert ds.size() == (2, 1, 1, 2, 1)
        _fold_and_check(ds, tr, [], [])  # an empty fold forgets the emissions, not the state
        assert ds.size() == (2, 1, 1, 0, 0) and len(ds.new_edges()[0]) == 0
        _check_state(ds, tr)
    with gs.Distinct(mode=mode) as ds:  # a loop: one vertex, one edge
        tr = Truth(mode)
        _fold_and_check(ds, tr, [4], [4])
        assert ds.size() == (1, 1, 1, 1, 1)
        _check_state(ds, tr)
    with gs.Distinct(mode=mode) as ds:  # the same edge twice in one fold: index 0 is kept
        tr = Truth(mode)
        assert _fold_and_check(ds, tr, [3, 3], [8, 8]) == [0]
        _check_state(ds, tr)


def test_reversed_edge_in_both_modes(gs):
    with gs.Distinct(mode="directed") as ds:
        ds.fold([7, 2], [2, 7])
        assert ds.size()[:2] == (2, 2)
        assert [x.tolist() for x in ds.edges()] == [[7, 2], [2, 7], [0, 1]]
    with gs.Distinct(mode="undirected") as ds:  # one edge, kept with its first orientation
        ds.fold([7, 2], [2, 7])
        assert ds.size()[:2] == (2, 1)
        assert [x.tolist() for x in ds.new_edges()] == [[0], [7], [2]]
        assert [x.tolist() for x in ds.edges()] == [[7], [2], [0]]
        ds.fold([2], [7])
        assert ds.size() == (2, 1, 3, 0, 0)


@pytest.mark.parametrize("mode", MODES)
def test_extreme_ids(gs, mode):
    src = [I64_MIN, I64_MAX, -1, 0, I64_MIN, I64_MAX, 0, I64_MIN]
    dst = [I64_MAX, I64_MIN, 0, -1, I64_MIN, I64_MAX, I64_MIN, 0]
    with gs.Distinct(mode=mode) as ds:
        tr = Truth(mode)
        _fold_and_check(ds, tr, src[:3], dst[:3])
        _fold_and_check(ds, tr, src[3:], dst[3:])
        assert ds.vertices().tolist() == [I64_MIN, I64_MAX, -1, 0]
        _check_state(ds, tr)


# ---- 3. tiles
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("mode", MODES)
def test_tiles_all_distinct_and_all_equal(gs, mode, n):
    with gs.Distinct(mode=mode) as ds:
        tr = Truth(mode)
        i = np.arange(n, dtype=np.int64)
        assert _fold_and_check(ds, tr, 10 + 2 * i, 11 + 2 * i) == list(range(n))
        assert ds.stats()["tiles"] == -(-n // T)
        _check_state(ds, tr)
    with gs.Distinct(mode=mode) as ds:  # one address takes every atomic
        tr = Truth(mode)
        assert _fold_and_check(ds, tr, np.full(n, 6), np.full(n, 3)) == [0]
        assert ds.stats()["tiles"] == -(-n // T)
        _check_state(ds, tr)


@pytest.mark.parametrize("mode", MODES)
def test_duplicate_one_tile_later(gs, mode):
    i = np.arange(T, dtype=np.int64)
    src, dst = np.concatenate([i, i]), np.concatenate([i + 1, i + 1])
    with gs.Distinct(mode=mode) as ds:
        tr = Truth(mode)
        assert _fold_and_check(ds, tr, src, dst) == list(range(T))
        assert ds.stats()["tiles"] == 2
        _check_state(ds, tr)


@pytest.mark.parametrize("pos", [T - 1, T])
@pytest.mark.parametrize("mode", MODES)
def test_only_new_edge_at_a_tile_end(gs, mode, pos):
    n = 2 * T
    src, dst = np.full(n, 1, np.int64), np.full(n, 2, np.int64)
    with gs.Distinct(mode=mode) as ds:
        tr = Truth(mode)
        _fold_and_check(ds, tr, [1], [2])
        src[pos], dst[pos] = 2, 3  # vertex 3 is new at entry 2 * pos + 1
        assert _fold_and_check(ds, tr, src, dst) == [pos]
        assert ds.new_vertices()[1].tolist() == [2 * pos + 1]
        _check_state(ds, tr)


@pytest.mark.parametrize("mode", MODES)
def test_run_of_one_edge_at_a_wave_boundary(gs, mode):
    n = 256
    src, dst = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64) + 1000
    src[32:96], dst[32:96] = 77, 78  # 64 consecutive copies across the boundary of waves 0 and 1
    with gs.Distinct(mode=mode) as ds:
        tr = Truth(mode)
        idx = _fold_and_check(ds, tr, src, dst)
        assert 32 in idx and not set(range(33, 96)) & set(idx)
        _check_state(ds, tr)


# ---- 4. cut-invariance
def _streams():
    rng = np.random.default_rng(0xD157)
    n = 1 << 15
    dense = (rng.integers(0, 1 << 10, n), rng.integers(0, 1 << 10, n))
    pool = rng.integers(I64_MIN, I64_MAX, 1 << 12, dtype=np.int64, endpoint=True)
    wide = (pool[rng.integers(0, len(pool), n)], rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True))
    return {"dense": dense, "wide": wide}


_STREAMS = _streams()
_WHOLE = {}


def _whole_truth(name, mode):
    """The truth of a stream folded whole: computed once, shared, left unchanged."""
    if (name, mode) not in _WHOLE:
        tr = Truth(mode)
        emitted = tr.fold(*_STREAMS[name])
        _WHOLE[(name, mode)] = (tr, emitted)
    return _WHOLE[(name, mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["dense", "wide"])
def test_cut_invariance(gs, name, mode):
    src, dst = _STREAMS[name]
    tr, ((nv, nent), idx) = _whole_truth(name, mode)
    with gs.Distinct(mode=mode) as ds:
        assert ds.fold(src, dst) == (len(nv), len(idx))
        assert ds.new_vertices()[0].tolist() == nv and ds.new_vertices()[1].tolist() == nent
        assert ds.new_edges()[0].tolist() == idx
        _check_state(ds, tr)
        whole = (ds.vertices(), ds.edges(), ds.size()[:3])
    rng = np.random.default_rng(7)
    cuts = np.sort(rng.integers(0, len(src) + 1, 12))
    cuts = np.concatenate([[0, 0], cuts, [cuts[5]], [len(src), len(src)]])  # empty folds included
    cuts.sort()
    with gs.Distinct(mode=mode) as ds:
        all_v, all_ent, all_idx = [], [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            ds.fold(src[a:b], dst[a:b])
            v, ent = ds.new_vertices()
            all_v += v.tolist()
            all_ent += (ent.astype(np.int64) + 2 * a).tolist()
            all_idx += (ds.new_edges()[0].astype(np.int64) + a).tolist()
        assert all_v == nv and all_ent == nent and all_idx == idx
        assert np.array_equal(ds.vertices(), whole[0])
        for x, y in zip(ds.edges(), whole[1]):
            assert np.array_equal(x, y)
        assert ds.size()[:3] == whole[2]
        _check_state(ds, tr)


# ---- 5. growth and probing
@pytest.mark.parametrize("mode", MODES)
def test_growth_and_probing(gs, mode):
    n = 3000
    with gs.Distinct(mode=mode, vertex_hint=0, edge_hint=0) as ds:
        tr = Truth(mode)
        before = ds.stats()
        assert before["vertex_rebuilds"] == 0 and before["edge_rebuilds"] == 0
        probes = []
        for f in range(4):  # dense ids 0 .. : every fold brings 2 n new vertices and n new edges
            i = np.arange(n, dtype=np.int64)
            src, dst = 2 * n * f + 2 * i, 2 * n * f + 2 * i + 1
            if f == 3:  # old vertices only; the edges reversed: old ones in undirected mode
                src, dst = np.asarray(tr.edst[:n]), np.asarray(tr.esrc[:n])
            _fold_and_check(ds, tr, src, dst)
            _check_state(ds, tr)
            probes.append(ds.stats()["longest_probe"])
        st = ds.stats()
        assert st["vertex_rebuilds"] >= 2 and st["edge_rebuilds"] >= 2
        assert st["vertex_slots"] >= 2 * len(tr.vlist) and st["edge_slots"] >= 2 * len(tr.esrc)
        assert st["vertex_slots"] > before["vertex_slots"] and st["edge_slots"] > before["edge_slots"]
        assert max(probes[:3]) >= 1


def test_profiled_fold_counts_its_atomics(gs):
    """Under the benchmark's knob a fold reports the occurrences that issued an atomic minimum:
    every occurrence of an all-distinct batch (2 n entries + n edges), none in the steady state."""
    n = T + 5
    i = np.arange(n, dtype=np.int64)
    with gs.Distinct() as ds:
        ds.fold(2 * i, 2 * i + 1)
        assert ds.phases()["atomics"] == 0 and ds.phases()["occurrences"] == 3 * n  # not profiled
        ds.reset()
        with gs.testing(distinct_profile=1):
            assert ds.fold(2 * i, 2 * i + 1) == (2 * n, n)
            assert ds.phases()["atomics"] == 3 * n == ds.phases()["occurrences"]
            assert ds.fold(2 * i, 2 * i + 1) == (0, 0)  # all old: no atomic at all
            assert ds.phases()["atomics"] == 0
            assert ds.fold(np.full(n, 1 << 40), np.full(n, 1 << 41)) == (2, 1)  # one key, many occurrences
            assert 3 <= ds.phases()["atomics"] <= 3 * n


# ---- 6. probes
@pytest.mark.parametrize("mode", MODES)
def test_contains_and_rank(gs, mode):
    import torch
    dev = "cuda:0"
    rng = np.random.default_rng(11)
    n = 4000
    src, dst = rng.integers(0, 300, n), rng.integers(0, 300, n)
    with gs.Distinct(mode=mode) as ds:
        tr = Truth(mode)
        ds.fold(src[:n // 2], dst[:n // 2])
        ds.fold(src[n // 2:], dst[n // 2:])
        tr.fold(src, dst)
        qs = np.concatenate([src, dst, rng.integers(0, 320, n), [I64_MIN, 5]])  # present, reversed, mixed, absent
        qd = np.concatenate([dst, src, rng.integers(0, 320, n), [5, I64_MAX]])
        want = [(int((s, d) in tr.keys or (mode == "undirected" and (d, s) in tr.keys))) for s, d in
                zip(qs.tolist(), qd.tolist())]
        found = torch.full((len(qs),), 9, dtype=torch.uint8, device=dev)
        dqs, dqd = torch.from_numpy(qs).to(dev), torch.from_numpy(qd).to(dev)
        ds.wait_stream("torch")
        ds.contains_device(dqs, dqd, found)
        ds.sync()
        assert found.cpu().tolist() == want
        assert 0 < sum(want[n:2 * n]) and (mode == "undirected") == all(want[n:2 * n])
        # ranks: the position in vertices(); absent ids give -1 and 0
        vs = ds.vertices()
        assert vs.tolist() == tr.vlist
        q = np.concatenate([vs, [1 << 40, -7, I64_MIN]])
        rank = torch.full((len(q),), 99, dtype=torch.int64, device=dev)
        fnd = torch.full((len(q),), 9, dtype=torch.uint8, device=dev)
        dq = torch.from_numpy(q).to(dev)
        ds.wait_stream("torch")
        ds.rank_device(dq, rank, fnd)
        ds.rank_device(dq, rank)  # found may be omitted
        ds.sync()
        assert rank.cpu().tolist() == list(range(len(vs))) + [-1, -1, -1]
        assert fnd.cpu().tolist() == [1] * len(vs) + [0, 0, 0]


def test_rank_equals_relabel_first_appearance(gs):
    import torch
    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(5)
    n, bound = 1 << 14, 5000
    src = torch.randint(0, bound, (n,), generator=g, dtype=torch.int64).to(dev)
    dst = torch.randint(0, bound, (n,), generator=g, dtype=torch.int64).to(dev)
    rs, rd = src.clone(), dst.clone()
    gs.relabel_first_appearance(rs, rd, bound)  # 1-based, torch scatter ops
    torch.cuda.synchronize()
    with gs.Distinct() as ds:
        ds.fold_device(src, dst, after="torch")
        ks, kd = torch.empty_like(src), torch.empty_like(dst)
        ds.rank_device(src, ks)
        ds.rank_device(dst, kd)
        ds.sync()
        assert torch.equal(ks, rs - 1) and torch.equal(kd, rd - 1)


# ---- 7. device path and lifetime
@pytest.mark.parametrize("mode", MODES)
def test_device_path_interleaved(gs, mode):
    import torch
    dev = "cuda:0"
    rng = np.random.default_rng(3)
    n = T + 77
    src, dst = rng.integers(-50, 50, n), rng.integers(-50, 50, n)
    inter = torch.from_numpy(np.stack([src, dst], 1).ravel().copy()).to(dev)  # s0 d0 s1 d1 ...
    torch.cuda.synchronize()
    tr = Truth(mode)
    (nv, nent), idx = tr.fold(src, dst)
    with gs.Distinct(mode=mode) as ds:
        assert ds.fold_device(inter, inter[1:], n=n, stride=2) == (len(nv), len(idx))
        gi = torch.empty(n, dtype=torch.int32, device=dev)
        es = torch.empty(n, dtype=torch.int64, device=dev)
        ed = torch.empty(n, dtype=torch.int64, device=dev)
        assert ds.new_edges_device(gi, es, ed) == len(idx)
        gv = torch.empty(2 * n, dtype=torch.int64, device=dev)
        ge = torch.empty(2 * n, dtype=torch.int32, device=dev)
        assert ds.new_vertices_device(gv, ge) == len(nv)
        av = torch.empty(len(tr.vlist), dtype=torch.int64, device=dev)
        assert ds.vertices_device(av) == len(tr.vlist)
        xs = torch.empty(len(idx), dtype=torch.int64, device=dev)
        xd = torch.empty(len(idx), dtype=torch.int64, device=dev)
        xf = torch.empty(len(idx), dtype=torch.int64, device=dev)
        assert ds.edges_device(xs, xd, xf) == len(idx)
        assert ds.edges_device(None, xd, None, cap=len(idx)) == len(idx)  # each array may be omitted
        ds.sync()
        assert gi[:len(idx)].cpu().tolist() == idx
        assert es[:len(idx)].cpu().tolist() == tr.esrc and ed[:len(idx)].cpu().tolist() == tr.edst
        assert gv[:len(nv)].cpu().tolist() == nv and ge[:len(nv)].cpu().tolist() == nent
        assert av.cpu().tolist() == tr.vlist
        assert xs.cpu().tolist() == tr.esrc and xd.cpu().tolist() == tr.edst and xf.cpu().tolist() == tr.efirst


def test_truncated_leaves_the_arrays_alone(gs):
    L = gs.lib()
    with gs.Distinct() as ds:
        ds.fold([1, 2, 3], [2, 3, 4])
        sent = -0x5A5A5A5A5A5A5A5B
        a = np.full(8, sent, np.int64)
        b = np.full(8, sent, np.int64)
        f = np.full(8, 0xA5A5A5A5A5A5A5A5, np.uint64)
        i = np.full(8, 0xA5A5A5A5, np.uint32)
        n = ctypes.c_size_t(0)
        calls = (
            (lambda: L.gs_distinct_new_edges(ds.handle, i.ctypes.data, a.ctypes.data, b.ctypes.data, 2, ctypes.byref(n)), 3),
            (lambda: L.gs_distinct_new_vertices(ds.handle, a.ctypes.data, i.ctypes.data, 3, ctypes.byref(n)), 4),
            (lambda: L.gs_distinct_vertices(ds.handle, a.ctypes.data, 0, ctypes.byref(n)), 4),
            (lambda: L.gs_distinct_edges(ds.handle, a.ctypes.data, b.ctypes.data, f.ctypes.data, 1, ctypes.byref(n)), 3),
        )
        for call, need in calls:
            n.value = 0
            assert call() == gs.GS_ERR_TRUNCATED
            assert n.value == need
            assert (a == sent).all() and (b == sent).all() and (f == 0xA5A5A5A5A5A5A5A5).all() and (i == 0xA5A5A5A5).all()
        assert L.gs_distinct_edges(ds.handle, a.ctypes.data, b.ctypes.data, f.ctypes.data, 3, ctypes.byref(n)) == gs.GS_OK
        assert a[:3].tolist() == [1, 2, 3] and a[3] == sent and f[:3].tolist() == [0, 1, 2]


@pytest.mark.parametrize("mode", MODES)
def test_reset_then_the_same_stream(gs, mode):
    rng = np.random.default_rng(19)
    src, dst = rng.integers(0, 500, 5000), rng.integers(0, 500, 5000)
    with gs.Distinct(mode=mode) as ds:
        tr = Truth(mode)
        _fold_and_check(ds, tr, src, dst)
        first = (ds.new_vertices(), ds.new_edges(), ds.vertices(), ds.edges(), ds.size())
        slots = ds.stats()["vertex_slots"], ds.stats()["edge_slots"]
        ds.reset()
        assert ds.size() == (0, 0, 0, 0, 0) and len(ds.vertices()) == 0 and len(ds.edges()[0]) == 0
        assert (ds.stats()["vertex_slots"], ds.stats()["edge_slots"]) == slots  # capacity is kept
        _fold_and_check(ds, Truth(mode), src, dst)
        again = (ds.new_vertices(), ds.new_edges(), ds.vertices(), ds.edges(), ds.size())
        for x, y in zip(first[:4], again[:4]):
            for p, q in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
                assert np.array_equal(p, q)
        assert first[4] == again[4]


def test_hbm_bytes_return_after_close(gs):
    start = gs.hbm_bytes(0)
    ds = gs.Distinct(vertex_hint=1 << 12, edge_hint=1 << 12)
    assert gs.hbm_bytes(0) > start
    rng = np.random.default_rng(23)
    ds.fold(rng.integers(0, 1 << 20, 20000), rng.integers(0, 1 << 20, 20000))  # grows tables and scratch
    ds.edges()
    held = gs.hbm_bytes(0)
    assert held > start
    ds.close()
    assert gs.hbm_bytes(0) == start


def test_mode_is_validated(gs):
    with pytest.raises(KeyError):
        gs.Distinct(mode="sideways")
    with pytest.raises(gs.GSError) as e:
        gs.Distinct(mode=2)
    assert e.value.code == gs.GS_ERR_INVALID
    with gs.Distinct(mode=1) as ds:
        assert ds.mode == gs.DISTINCT_MODES["undirected"]


# ---- 8. composition: the reason for the feature
def test_degrees_of_the_simple_graph(gs):
    rng = np.random.default_rng(29)
    n = 1 << 14
    src = rng.integers(0, 400, n)
    dst = (src + 1 + rng.integers(0, 399, n)) % 400  # no loops; repeated and reversed edges in plenty
    neighbours = {}
    for s, d in zip(src.tolist(), dst.tolist()):
        neighbours.setdefault(s, set()).add(d)
        neighbours.setdefault(d, set()).add(s)
    with gs.Distinct(mode="undirected") as ds, gs.Degrees("all", capacity_hint=1 << 10) as dg:
        for a in range(0, n, 5000):
            ds.fold(src[a:a + 5000], dst[a:a + 5000])
            idx = ds.new_edges()[0]
            dg.fold(src[a:a + 5000][idx], dst[a:a + 5000][idx])
        v, deg = dg.degrees(sorted=True)
        assert v.tolist() == sorted(neighbours) and deg.tolist() == [len(neighbours[x]) for x in sorted(neighbours)]
        assert ds.size()[1] == sum(deg.tolist()) // 2 < n


def test_triangles_of_the_kept_edges(gs):
    rng = np.random.default_rng(31)
    n = 1 << 13
    src, dst = rng.integers(0, 200, n), rng.integers(0, 200, n)
    with gs.Distinct(mode="undirected") as ds, gs.Triangles(edge_hint=n) as kept, gs.Triangles(edge_hint=n) as full:
        ds.fold(src, dst)
        idx = ds.new_edges()[0]
        assert 0 < len(idx) < n
        kept.fold(src[idx], dst[idx])
        full.fold(src, dst)
        assert kept.count() == full.count() and kept.count()[0] > 0
        for x, y in zip(kept.local_counts(), full.local_counts()):
            assert np.array_equal(x, y)


# ---- more tiles than one step (edges) and two steps (entries) of the tile-count scan
@pytest.mark.parametrize("edges", ["all-distinct", "all-equal"])
def test_tile_scan_past_its_steps(gs, edges):
    """One fold of T * TILE_SCAN_BLOCK + 1 edges: the edge compaction scans one tile count more
    than a step of gsamd.TILE_SCAN_BLOCK, the vertex compaction one more than two steps; the
    bases of the later tiles are sums the scan carries from step to step."""
    n = gsamd.TILE_SCAN_BLOCK * T + 1
    i = np.arange(n, dtype=np.int64)
    src, dst = (2 * i, 2 * i + 1) if edges == "all-distinct" else (np.full(n, 5, np.int64), np.full(n, 9, np.int64))
    assert -(-n // T) == gsamd.TILE_SCAN_BLOCK + 1 and -(-2 * n // T) == 2 * gsamd.TILE_SCAN_BLOCK + 1
    entries = np.stack([src, dst], axis=1).ravel()  # entry 2 i = src, 2 i + 1 = dst of edge i
    new_entry = np.sort(np.unique(entries, return_index=True)[1])
    kept = np.sort(np.unique((src << 32) | dst, return_index=True)[1])  # (ids below 2^31)
    with gs.Distinct(vertex_hint=len(new_entry), edge_hint=len(kept)) as ds:
        assert ds.fold(src, dst) == (len(new_entry), len(kept))
        assert ds.stats()["tiles"] == gsamd.TILE_SCAN_BLOCK + 1
        v, ent = ds.new_vertices()
        assert np.array_equal(v, entries[new_entry]) and np.array_equal(ent, new_entry)
        assert np.array_equal(ds.new_edges()[0], kept)
