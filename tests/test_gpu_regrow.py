"""GPU: every buffer group of a stand-alone summary handle regrowing several times in one life.
Each handle is created with the smallest hint its constructor accepts and is fed batches of 1, 3,
700 and 5000 edges over at most 256 vertex ids -- each more than 1.5 times the one before, so
every group with a quarter or a half of headroom has to grow at every batch -- with the host-array
exports and queries called between the folds, so that their staging groups grow too. Every result
is compared with the CPU model of the summary's own GPU test (test_gpu_triangles._truth,
test_gpu_slice._truth, test_gpu_distinct.Truth, test_gpu_spanner.Model, test_gpu_matching.Model).
Everything is an integer: every comparison is exact."""
import numpy as np
import pytest

import test_gpu_distinct
import test_gpu_matching
import test_gpu_slice
import test_gpu_spanner
import test_gpu_triangles

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 700, 5000)
IDS = 256


def _batches(seed, with_val=False):
    rng = np.random.default_rng(seed)
    for n in BATCHES:
        src = rng.integers(0, IDS, n, dtype=np.int64)
        dst = rng.integers(0, IDS, n, dtype=np.int64)
        yield (src, dst, rng.integers(0, 1000, n, dtype=np.int64)) if with_val else (src, dst)


def test_triangles(gs):
    all_s, all_d = np.zeros(0, np.int64), np.zeros(0, np.int64)
    with gs.Triangles(edge_hint=0) as tr:
        for src, dst in _batches(1):
            tr.fold(src, dst)
            all_s, all_d = np.concatenate([all_s, src]), np.concatenate([all_d, dst])
            ids, t, total, edges = test_gpu_triangles._truth(all_s, all_d)
            assert tr.count() == (total, edges, len(ids))
            v, c = tr.local_counts()
            assert np.array_equal(v, ids) and np.array_equal(c, t)
            v, c = tr.local_counts(nonzero_only=True)
            assert np.array_equal(v, ids[t > 0]) and np.array_equal(c, t[t > 0])


@pytest.mark.parametrize("direction", ("out", "all"))
def test_slice(gs, direction):
    with gs.Slice(edge_hint=0) as sl:
        for src, dst, val in _batches(2, with_val=True):
            test_gpu_slice._check(sl, src, dst, val, direction)  # window, every reduce, neighborhoods


@pytest.mark.parametrize("mode", test_gpu_distinct.MODES)
def test_distinct(gs, mode):
    truth = test_gpu_distinct.Truth(mode)
    with gs.Distinct(mode=mode, vertex_hint=0, edge_hint=0) as ds:
        for src, dst in _batches(3):
            test_gpu_distinct._fold_and_check(ds, truth, src, dst)  # the fold, new_vertices, new_edges
            test_gpu_distinct._check_state(ds, truth)  # vertices, edges
        assert ds.stats()["vertex_rebuilds"] >= 1 and ds.stats()["edge_rebuilds"] >= 1


def test_spanner(gs):
    model = test_gpu_spanner.Model(3)
    rng = np.random.default_rng(4)
    with gs.Spanner(k=3, edge_hint=0) as sp:
        for src, dst in _batches(5):
            assert sp.fold(src, dst).tolist() == model.fold(src.tolist(), dst.tolist())
            lo, hi = sp.edges()
            assert list(zip(lo.tolist(), hi.tolist())) == model.edges()
            assert sp.count()[0] == len(lo)
            # as many queries as the batch had edges: the query staging is the fold's scratch
            qs, qd = rng.integers(0, IDS + 8, len(src)), rng.integers(0, IDS + 8, len(src))
            for k in (1, 3):
                want = [model.within(s, t, k) for s, t in zip(qs.tolist(), qd.tolist())]
                assert sp.within(qs, qd, k).tolist() == want


def test_matching(gs):
    import torch
    dev = torch.device("cuda:0")
    model = test_gpu_matching.Model()
    seen = set()
    with gs.Matching(vertex_hint=0) as m:
        for (src, dst, val), queries in zip(_batches(6, with_val=True), (1, 2000, 1, 2000)):
            acc, events = model.fold(src.tolist(), dst.tolist(), val.tolist())
            assert m.fold(src, dst, val).tolist() == acc
            assert test_gpu_matching._events_of(m) == events
            edges = model.edges()
            assert test_gpu_matching._edges_of(m) == [tuple(e) for e in edges]
            seen |= set(src.tolist()) | set(dst.tolist())
            assert m.count() == (len(edges), len(seen), model.weight())
            ids = (np.arange(queries, dtype=np.int64) * 7) % (IDS + 64)  # present, unmatched and absent ids
            q = torch.from_numpy(ids).to(dev)
            mate = torch.full((queries,), -5, dtype=torch.int64, device=dev)
            value = torch.full((queries,), -5, dtype=torch.int64, device=dev)
            found = torch.full((queries,), 7, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            m.mate_device(q, mate, value, found)
            m.sync()
            want = [model.at.get(x) for x in ids.tolist()]
            assert found.cpu().tolist() == [1 if e else 0 for e in want]
            partner = [(e[1] if x == e[0] else e[0]) if e else 0 for x, e in zip(ids.tolist(), want)]
            assert mate.cpu().tolist() == partner
            assert value.cpu().tolist() == [e[2] if e else 0 for e in want]

