"""GPU: the host-array forms of the stand-alone summaries against their device forms. Every
handle type folds the same stream twice, one handle through host arrays and one through device
arrays, first 1 edge and then 2049 (one past the 2048-position tile; the second call also grows
every stage the first one sized), and every export of the host form must equal the device form's.
For one export per handle: a None column leaves the others as they are, and a capacity one below
the row count gives GS_ERR_TRUNCATED with the row count still reported. Last, the one-column sort
behind Distinct.edges and Matching.edges: after 300 folded edges (above 256: two passes under
either bound) the rows are in arrival order. Every output is an integer: comparisons are exact."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 2049)
IDS = 64  # a dense graph: repeats, triangles and matched vertices at both sizes


def _stream(n, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, IDS, n).astype(np.int64)
    dst = rng.integers(0, IDS, n).astype(np.int64)
    val = rng.integers(1, 1 << 20, n).astype(np.int64)
    return src, dst, val


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _empty(torch, n, dtype):
    """a device array of n elements of a numpy dtype, read back with _back"""
    t = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[np.dtype(dtype).itemsize]
    return torch.zeros(max(n, 1), dtype=t, device=torch.device("cuda", 0))


def _back(t, n, dtype):
    return t.cpu().numpy().view(dtype)[:n].copy()


def _same(host, dev):
    assert len(host) == len(dev)
    for a, b in zip(host, dev):
        assert a.dtype == b.dtype and np.array_equal(a, b), (a[:8], b[:8])


def _host_call(gs, fn, h, cols, cap):
    """fn(handle, *columns, cap, &n) with numpy columns (None: a null pointer); returns (rc, n)"""
    got = ctypes.c_size_t(0)
    rc = fn(h._h, *[None if c is None else c.ctypes.data for c in cols], cap, ctypes.byref(got))
    return rc, got.value


def _none_and_truncated(gs, fn, h, full, drop):
    """full: the host form's columns with every column given. Without column `drop` the others are
    the same; with capacity rows - 1 the call is truncated and still reports the rows."""
    rows = len(full[0])
    assert rows > 0
    cols = [None if i == drop else np.zeros(rows, c.dtype) for i, c in enumerate(full)]
    rc, n = _host_call(gs, fn, h, cols, rows)
    assert rc == gs.GS_OK and n == rows
    for i, c in enumerate(cols):
        if c is not None:
            assert np.array_equal(c, full[i]), i
    cols = [np.zeros(rows, c.dtype) for c in full]
    rc, n = _host_call(gs, fn, h, cols, rows - 1)
    assert rc == gs.GS_ERR_TRUNCATED and n == rows
    assert all(not c.any() for c in cols)  # nothing was written


def test_distinct_host_and_device_forms(gs):
    import torch
    H, D = gs.Distinct(mode="undirected"), gs.Distinct(mode="undirected")
    for n in SIZES:
        src, dst, _ = _stream(n, 11 + n)
        ts, td = _dev(torch, src), _dev(torch, dst)
        assert H.fold(src, dst) == D.fold_device(ts, td, after="torch")
        assert H.size() == D.size()
        nv, ne, _, new_v, new_e = D.size()
        idx, s, d = (_empty(torch, new_e, t) for t in (np.uint32, np.int64, np.int64))
        assert D.new_edges_device(idx, s, d) == new_e
        v, ent = _empty(torch, new_v, np.int64), _empty(torch, new_v, np.uint32)
        assert D.new_vertices_device(v, ent) == new_v
        av = _empty(torch, nv, np.int64)
        assert D.vertices_device(av) == nv
        es, ed, ef = (_empty(torch, ne, t) for t in (np.int64, np.int64, np.uint64))
        assert D.edges_device(es, ed, ef) == ne
        D.sync()
        _same(H.new_edges(), [_back(idx, new_e, np.uint32), _back(s, new_e, np.int64), _back(d, new_e, np.int64)])
        _same(H.new_vertices(), [_back(v, new_v, np.int64), _back(ent, new_v, np.uint32)])
        _same([H.vertices()], [_back(av, nv, np.int64)])
        _same(H.edges(), [_back(es, ne, np.int64), _back(ed, ne, np.int64), _back(ef, ne, np.uint64)])
    _none_and_truncated(gs, gs.lib().gs_distinct_edges, H, H.edges(), drop=1)
    H.close()
    D.close()


def test_matching_host_and_device_forms(gs):
    import torch
    H, D = gs.Matching(vertex_hint=16), gs.Matching(vertex_hint=16)
    for n in SIZES:
        src, dst, val = _stream(n, 23 + n)
        acc = _empty(torch, n, np.uint8)
        D.fold_device(_dev(torch, src), _dev(torch, dst), _dev(torch, val), accepted=acc, after="torch")
        D.sync()
        assert np.array_equal(H.fold(src, dst, val), _back(acc, n, np.uint8).astype(bool))
        assert H.count() == D.count()
        events = H.events()
        k = len(events[0])
        cols = [_empty(torch, k, t) for t in (np.uint32, np.uint8, np.int64, np.int64, np.int64)]
        assert D.events_device(*cols) == k
        ne = D.count()[0]
        exp = [_empty(torch, ne, t) for t in (np.int64, np.int64, np.int64, np.uint64)]
        assert D.edges_device(*exp) == ne
        D.sync()
        _same(events, [_back(c, k, t) for c, t in zip(cols, (np.uint32, np.uint8, np.int64, np.int64, np.int64))])
        _same(H.edges(), [_back(c, ne, t) for c, t in zip(exp, (np.int64, np.int64, np.int64, np.uint64))])
    _none_and_truncated(gs, gs.lib().gs_matching_export, H, H.edges(), drop=2)
    H.close()
    D.close()


def test_degree_stream_host_and_device_forms(gs):
    import torch
    H, D = gs.DegreeStream(vertex_hint=16), gs.DegreeStream(vertex_hint=16)
    for n in SIZES:
        src, dst, val = _stream(n, 37 + n)
        dele = None if n == 1 else (val % 5 == 0).astype(np.uint8)  # the byte column: absent, then given
        H.fold(src, dst, deletions=dele)
        D.fold_device(_dev(torch, src), _dev(torch, dst), deletions=None if dele is None else _dev(torch, dele),
                      after="torch")
        assert H.size() == D.size()
        occ, rec = D.size()["occurrences"], D.size()["records"]
        rows = [_empty(torch, occ, t) for t in (np.int64, np.uint32, np.uint32)]
        assert D.rows_device(*rows) == occ
        recs = [_empty(torch, rec, np.uint32) for _ in range(3)]
        assert D.records_device(*recs) == rec
        hd, hdist = H.degrees(sorted=False), H.distribution()
        deg = [_empty(torch, len(hd[0]), np.int64) for _ in range(2)]
        assert D.degrees_device(*deg) == len(hd[0])
        dist = [_empty(torch, len(hdist[0]), np.int64) for _ in range(2)]
        assert D.distribution_device(*dist) == len(hdist[0])
        D.sync()
        _same(H.rows(), [_back(c, occ, t) for c, t in zip(rows, (np.int64, np.uint32, np.uint32))])
        _same(H.records(), [_back(c, rec, np.uint32) for c in recs])
        _same(hd, [_back(c, len(hd[0]), np.int64) for c in deg])
        _same(hdist, [_back(c, len(hdist[0]), np.int64) for c in dist])
    _none_and_truncated(gs, gs.lib().gs_degstream_degrees, H, H.degrees(sorted=False), drop=0)
    H.close()
    D.close()


def test_triangle_stream_host_and_device_forms(gs):
    import torch
    H, D = gs.TriangleStream(), gs.TriangleStream()
    for n in SIZES:
        src, dst, _ = _stream(n, 41 + n)
        H.fold(src, dst)
        D.fold_device(_dev(torch, src), _dev(torch, dst), after="torch")
        assert H.size() == D.size() and H.count() == D.count()
        rec = D.size()["records"]
        rows = [_empty(torch, n, np.uint32), _empty(torch, n, np.int64)]
        assert D.rows_device(*rows) == n
        recs = [_empty(torch, rec, t) for t in (np.uint32, np.int64, np.int64)]
        assert D.records_device(*recs) == rec
        hc = H.local_counts()
        cnt = [_empty(torch, len(hc[0]), np.int64) for _ in range(2)]
        assert D.local_counts_device(*cnt) == len(hc[0])
        D.sync()
        _same(H.rows(), [_back(rows[0], n, np.uint32), _back(rows[1], n, np.int64)])
        _same(H.records(), [_back(c, rec, t) for c, t in zip(recs, (np.uint32, np.int64, np.int64))])
        _same(hc, [_back(c, len(hc[0]), np.int64) for c in cnt])
    _none_and_truncated(gs, gs.lib().gs_tristream_counts, H, H.local_counts(), drop=0)
    H.close()
    D.close()


def test_slice_host_and_device_forms(gs):
    import torch
    H, D = gs.Slice(), gs.Slice()
    for n in SIZES:
        src, dst, val = _stream(n, 53 + n)
        H.window(src, dst, val, direction="all")
        D.window_device(_dev(torch, src), _dev(torch, dst), _dev(torch, val), direction="all", after="torch")
        assert H.size() == D.size()
        nv, ne = D.size()
        rv, ro = _empty(torch, nv, np.int64), _empty(torch, nv, np.int64)
        assert D.reduce_device("sum", rv, ro) == nv
        v, off = _empty(torch, nv, np.int64), _empty(torch, nv + 1, np.uint64)
        nb, w = _empty(torch, ne, np.int64), _empty(torch, ne, np.int64)
        assert D.neighborhoods_device(v, off, nb, w) == (nv, ne)
        D.sync()
        _same(H.reduce("sum"), [_back(rv, nv, np.int64), _back(ro, nv, np.int64)])
        _same(H.neighborhoods(), [_back(v, nv, np.int64), _back(off, nv + 1, np.uint64), _back(nb, ne, np.int64),
                                  _back(w, ne, np.int64)])
    # neighborhoods without the optional val column; reduce one row short
    full = H.neighborhoods()
    nv, ne = H.size()
    got_v, got_e = ctypes.c_size_t(0), ctypes.c_size_t(0)
    v, off, nb = np.zeros(nv, np.int64), np.zeros(nv + 1, np.uint64), np.zeros(ne, np.int64)
    rc = gs.lib().gs_slice_neighborhoods(H._h, v.ctypes.data, off.ctypes.data, nb.ctypes.data, None, nv, ne,
                                         ctypes.byref(got_v), ctypes.byref(got_e))
    assert rc == gs.GS_OK and (got_v.value, got_e.value) == (nv, ne)
    _same(full[:3], [v, off, nb])
    rv, ro = np.zeros(nv, np.int64), np.zeros(nv, np.int64)
    rc = gs.lib().gs_slice_reduce(H._h, gs.SLICE_OPS["sum"], rv.ctypes.data, ro.ctypes.data, nv - 1, ctypes.byref(got_v))
    assert rc == gs.GS_ERR_TRUNCATED and got_v.value == nv and not rv.any() and not ro.any()
    H.close()
    D.close()


def test_triangle_sampler_host_and_device_forms(gs):
    import torch
    S = 256
    H, D = gs.TriangleSampler(samples=S, vertices=IDS), gs.TriangleSampler(samples=S, vertices=IDS)
    kinds = (np.int64, np.int64, np.int64, np.uint8, np.int32)
    for n in SIZES:
        src, dst, _ = _stream(n, 67 + n)
        assert H.fold(src, dst) == D.fold_device(_dev(torch, src), _dev(torch, dst), after="torch")
        assert H.estimate() == D.estimate()
        hr = H.rows()
        k = len(hr[0])
        rows = [_empty(torch, k, np.int32) for _ in range(3)]
        assert D.rows_device(*rows) == k
        st = [_empty(torch, S, t) for t in kinds]
        D.states_device(*st)
        D.sync()
        _same(hr, [_back(c, k, np.int32) for c in rows])
        _same(H.states(), [_back(c, S, t) for c, t in zip(st, kinds)])
    _none_and_truncated(gs, gs.lib().gs_trisample_rows, H, H.rows(), drop=1)
    # the states without two of their columns
    full = H.states()
    s, th, at = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int32)
    assert gs.lib().gs_trisample_states(H._h, s.ctypes.data, None, th.ctypes.data, None, at.ctypes.data) == gs.GS_OK
    _same([full[0], full[2], full[4]], [s, th, at])
    H.close()
    D.close()


def test_edges_after_300_folds_are_in_arrival_order(gs):
    """sort_by_key under the bound 2 * folded = 600 (Distinct) and folded = 300 (Matching): passes 0 and 1."""
    import torch
    n = 300
    src = np.arange(n, dtype=np.int64) * 7919 % 1009 + 5  # distinct ids (1009 is prime), not ascending
    dst = src + 5000
    val = np.arange(n, dtype=np.int64) + 1
    assert len(set(src.tolist())) == n
    H, D = gs.Distinct(), gs.Distinct()
    H.fold(src, dst)
    D.fold_device(_dev(torch, src), _dev(torch, dst), after="torch")
    es, ed, ef = (_empty(torch, n, t) for t in (np.int64, np.int64, np.uint64))
    assert D.edges_device(es, ed, ef) == n
    D.sync()
    dev = [_back(es, n, np.int64), _back(ed, n, np.int64), _back(ef, n, np.uint64)]
    _same(H.edges(), dev)
    assert np.array_equal(dev[0], src) and np.array_equal(dev[1], dst) and np.all(np.diff(dev[2].astype(np.int64)) > 0)
    H.close()
    D.close()
    # vertex-disjoint edges of positive value are all accepted, in arrival order
    H, D = gs.Matching(), gs.Matching()
    assert H.fold(src, dst, val).all()
    D.fold_device(_dev(torch, src), _dev(torch, dst), _dev(torch, val), after="torch")
    exp = [_empty(torch, n, t) for t in (np.int64, np.int64, np.int64, np.uint64)]
    assert D.edges_device(*exp) == n
    D.sync()
    dev = [_back(c, n, t) for c, t in zip(exp, (np.int64, np.int64, np.int64, np.uint64))]
    _same(H.edges(), dev)
    assert np.array_equal(dev[0], src) and np.array_equal(dev[1], dst) and np.array_equal(dev[2], val)
    assert np.all(np.diff(dev[3].astype(np.int64)) > 0)
    H.close()
    D.close()
