"""GPU: the degree summary (gsamd.Degrees, the gs_degree_* calls) against numpy -- the
authority: np.unique(..., return_counts=True) on the collected endpoints, additions minus
deletions -- and against the reference's pinned outputs (tests/golden/degree_pins.json).
Every output is an integer: comparisons are exact."""
import ctypes
import gc
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
SENTINEL = -0x5A5A5A5A5A5A5A5B
DIRS = ("all", "in", "out")


def _pins():
    with open(os.path.join(GOLD, "degree_pins.json")) as f:
        return json.load(f)


def _sizes(gs):
    T = gs.DEGREE_TILE
    return (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5)


def _net(src, dst, direction, dele=None):
    """(ids ascending, net count) of every collected endpoint: occurrences added minus deleted."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    dele = np.zeros(len(src), np.uint8) if dele is None else np.asarray(dele, np.uint8)
    ends = {"all": (src, dst), "out": (src,), "in": (dst,)}[direction]
    add = np.concatenate([e[(dele & 1) == 0] for e in ends])
    rem = np.concatenate([e[(dele & 1) == 1] for e in ends])
    ua, ca = np.unique(add, return_counts=True)
    ur, cr = np.unique(rem, return_counts=True)
    ids = np.union1d(ua, ur)
    net = np.zeros(len(ids), np.int64)
    net[np.searchsorted(ids, ua)] += ca
    net[np.searchsorted(ids, ur)] -= cr
    return ids, net


def _dev(gs_obj, a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(torch.device("cuda", gs_obj.device)) if dtype is None else t.to(dtype).to(
        torch.device("cuda", gs_obj.device))


def _fold_dev(D, src, dst, dele=None, **kw):
    """fold_device of numpy arrays staged through torch tensors (ordered behind torch's stream,
    and complete before the tensors are released)."""
    ts, td = _dev(D, src), _dev(D, dst)
    te = None if dele is None else _dev(D, dele)
    D.fold_device(ts, td, deletions=te, after="torch", **kw)
    D.sync()


def _check(D, ids, net, absent=()):
    """Every read of the summary D against the truth (ids ascending, net)."""
    import torch
    dev = torch.device("cuda", D.device)
    live = net > 0
    ev, ed = ids[live], net[live]
    # sorted export, host and device
    v, d = D.degrees(sorted=True)
    assert np.array_equal(v, ev) and np.array_equal(d, ed)
    n = len(ev)
    tv = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=dev)
    td = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=dev)
    D.wait_stream("torch")  # the buffers were filled on torch's stream
    assert D.degrees_device(tv, td, sorted=True) == n
    assert np.array_equal(tv[:n].cpu().numpy(), ev) and np.array_equal(td[:n].cpu().numpy(), ed)
    assert int(tv[n]) == SENTINEL and int(td[n]) == SENTINEL
    # unsorted export, as a set
    for v, d in (D.degrees(sorted=False),):
        o = np.argsort(v, kind="stable")
        assert np.array_equal(v[o], ev) and np.array_equal(d[o], ed)
    tv.fill_(SENTINEL)
    td.fill_(SENTINEL)
    D.wait_stream("torch")
    assert D.degrees_device(tv, td, sorted=False) == n
    uv, ud = tv[:n].cpu().numpy(), td[:n].cpu().numpy()
    o = np.argsort(uv, kind="stable")
    assert np.array_equal(uv[o], ev) and np.array_equal(ud[o], ed)
    # batched find: every id of the truth and the absent ones
    q = np.concatenate([ids, np.asarray(absent, np.int64)]).astype(np.int64)
    want = np.concatenate([np.where(live, net, 0), np.zeros(len(absent), np.int64)])
    if len(q):
        tq = _dev(D, q)
        tdeg = torch.full((len(q),), SENTINEL, dtype=torch.int64, device=dev)
        tf = torch.full((len(q),), 0xA5, dtype=torch.uint8, device=dev)
        D.wait_stream("torch")
        D.find_device(tq, tdeg, tf)
        D.sync()
        assert np.array_equal(tdeg.cpu().numpy(), want)
        assert np.array_equal(tf.cpu().numpy(), (want > 0).astype(np.uint8))
        tdeg.fill_(SENTINEL)
        D.wait_stream("torch")
        D.find_device(tq, tdeg, None)
        D.sync()
        assert np.array_equal(tdeg.cpu().numpy(), want)
    # distribution, host and device
    xd, xc = np.unique(ed, return_counts=True)
    gd, gc_ = D.distribution()
    assert np.array_equal(gd, xd) and np.array_equal(gc_, xc)
    assert np.all(gd[1:] > gd[:-1])
    k = len(xd)
    t1 = torch.full((k + 1,), SENTINEL, dtype=torch.int64, device=dev)
    t2 = torch.full((k + 1,), SENTINEL, dtype=torch.int64, device=dev)
    D.wait_stream("torch")
    assert D.distribution_device(t1, t2) == k
    assert np.array_equal(t1[:k].cpu().numpy(), xd) and np.array_equal(t2[:k].cpu().numpy(), xc)
    assert int(t1[k]) == SENTINEL and int(t2[k]) == SENTINEL


# ------------------------------------------------------------------ reference vectors
def _final_degrees(lines):
    """TestGetDegrees pins every value the continuous stream emits: {(v, i) : 1 <= i <= degree(v)}."""
    deg = {}
    for ln in lines:
        v, i = (int(x) for x in ln.split(","))
        deg[v] = max(deg.get(v, 0), i)
    expanded = sorted("%d,%d" % (v, i) for v, k in deg.items() for i in range(1, k + 1))
    assert expanded == sorted(lines)  # the final degrees expand to exactly the pinned lines
    ids = np.array(sorted(deg), np.int64)
    return ids, np.array([deg[int(v)] for v in ids], np.int64)


def _final_distribution(text):
    """DegreeDistribution pins every (degree, count) emitted: the last count per degree, zeros dropped."""
    last = {}
    for ln in text.split("\n"):
        d, c = (int(x) for x in ln.strip("()").split(","))
        last[d] = c
    ds = np.array(sorted(d for d, c in last.items() if c > 0), np.int64)
    return ds, np.array([last[int(d)] for d in ds], np.int64)


def _events(text):
    src, dst, dele = [], [], []
    for ln in text.split("\n"):
        a, b, s = ln.split()
        src.append(int(a))
        dst.append(int(b))
        dele.append(1 if s == "-" else 0)
    return np.array(src, np.int64), np.array(dst, np.int64), np.array(dele, np.uint8)


@pytest.mark.parametrize("per_edge", [False, True])
@pytest.mark.parametrize("name", ["get_degrees", "get_in_degrees", "get_out_degrees"])
def test_reference_get_degrees(gs, name, per_edge):
    pins = _pins()
    e = np.array(pins["sample_edges"]["edges"], np.int64)
    ids, deg = _final_degrees(pins[name]["lines"])
    with gs.Degrees(pins[name]["direction"], capacity_hint=16) as D:
        if per_edge:
            for s, d, _ in e:
                D.fold([s], [d])
        else:
            D.fold(e[:, 0], e[:, 1])
        v, d = D.degrees()
        assert np.array_equal(v, ids) and np.array_equal(d, deg)
        tids, tnet = _net(e[:, 0], e[:, 1], pins[name]["direction"])
        assert np.array_equal(tids, ids) and np.array_equal(tnet, deg)  # numpy agrees with the pin
        _check(D, ids, deg, absent=[0, 6, -1])


@pytest.mark.parametrize("per_edge", [False, True])
@pytest.mark.parametrize("data,result", [("degrees_data", "degrees_result"),
                                         ("degrees_data_zero", "degrees_result_zero")])
def test_reference_degree_distribution(gs, data, result, per_edge):
    pins = _pins()
    src, dst, dele = _events(pins[data]["text"])
    xd, xc = _final_distribution(pins[result]["text"])
    assert (dict(zip(xd.tolist(), xc.tolist())) ==
            ({1: 2, 2: 1} if data == "degrees_data" else {1: 1, 2: 1}))
    with gs.Degrees("all", capacity_hint=16) as D:
        if per_edge:
            for i in range(len(src)):
                D.fold(src[i:i + 1], dst[i:i + 1], dele[i:i + 1])
        else:
            D.fold(src, dst, dele)
        gd, gc_ = D.distribution()
        assert np.array_equal(gd, xd) and np.array_equal(gc_, xc)
        _check(D, *_net(src, dst, "all", dele), absent=[0, 5])


# ------------------------------------------------------------------ random sparse ids
def _sparse_edges(rng, n):
    pool = rng.integers(I64_MIN, I64_MAX, size=max(2, n // 2), dtype=np.int64, endpoint=True)
    pool = np.concatenate([pool, np.array([I64_MIN, I64_MAX, -1, 0, -(1 << 40)], np.int64)])
    src = pool[rng.integers(0, len(pool), n)]
    dst = pool[rng.integers(0, len(pool), n)]
    loops = rng.integers(0, n, max(1, n // 16))
    dst[loops] = src[loops]  # self-loops
    src[0] = I64_MIN if n > 1 else src[0]
    if n > 2:
        dst[1] = I64_MAX
        src[2] = dst[2] = I64_MIN  # a self-loop on the id that is the table's empty marker
    absent = np.setdiff1d(rng.integers(I64_MIN, I64_MAX, size=8, dtype=np.int64), np.concatenate([src, dst]))
    return src, dst, absent


@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("k", range(12))
def test_random_sparse_ids(gs, k, direction):
    n = _sizes(gs)[k]
    rng = np.random.default_rng(1000 + k)
    src, dst, absent = _sparse_edges(rng, n)
    ids, net = _net(src, dst, direction)
    # an endpoint that is not collected is never inserted: it is absent
    absent = np.concatenate([absent, np.setdiff1d(np.concatenate([src, dst]), ids)])
    with gs.Degrees(direction, capacity_hint=max(16, n)) as D:
        _fold_dev(D, src, dst)
        _check(D, ids, net, absent)
        assert D.num_vertices() == len(ids)


# ------------------------------------------------------------------ contention shapes
@pytest.mark.parametrize("direction", DIRS)
def test_star_and_self_loops(gs, direction):
    n = 3 * gs.DEGREE_TILE + 5
    hub = np.int64(-77)
    src = np.full(n, hub, np.int64)
    dst = np.arange(1, n + 1, dtype=np.int64) * 1000003
    with gs.Degrees(direction, capacity_hint=2 * n) as D:
        _fold_dev(D, src, dst)
        ids, net = _net(src, dst, direction)
        _check(D, ids, net)
        if direction != "in":
            assert net[np.searchsorted(ids, hub)] == n
    loop = np.full(n, 5, np.int64)
    with gs.Degrees(direction, capacity_hint=16) as D:
        _fold_dev(D, loop, loop)
        v, d = D.degrees()
        assert v.tolist() == [5] and d.tolist() == [2 * n if direction == "all" else n]
        _check(D, *_net(loop, loop, direction))


@pytest.mark.parametrize("direction", DIRS)
def test_hash_line_contention(gs, direction):
    """Eight ids 0..7 share one 128-byte line of the table (gs_device.hpp hash_slot)."""
    n = 3 * gs.DEGREE_TILE + 5
    rng = np.random.default_rng(7)
    src = rng.integers(0, 8, n).astype(np.int64)
    dst = rng.integers(0, 8, n).astype(np.int64)
    with gs.Degrees(direction, capacity_hint=16) as D:
        _fold_dev(D, src, dst)
        _check(D, *_net(src, dst, direction), absent=[8, 9, -1])


def test_on_chip_table_overflow(gs):
    """All-distinct ids: 2T distinct endpoints in one tile (more than fit the LDS hash's bounded
    probe), then three tiles of them; ids that find no on-chip slot take the global path."""
    T = gs.DEGREE_TILE
    rng = np.random.default_rng(11)
    for n in (T, 3 * T + 5):
        ids = rng.permutation(np.arange(1, 2 * n + 1, dtype=np.int64) * 7919 - (n << 20))
        src, dst = ids[:n].copy(), ids[n:].copy()
        with gs.Degrees("all", capacity_hint=2 * n) as D:
            _fold_dev(D, src, dst)
            tids, net = _net(src, dst, "all")
            assert len(tids) == 2 * n and np.all(net == 1)
            _check(D, tids, net)


def test_shared_id_at_the_tile_boundary(gs):
    T = gs.DEGREE_TILE
    ids = np.arange(1, 4 * T + 1, dtype=np.int64) * 104729
    src, dst = ids[:2 * T].copy(), ids[2 * T:].copy()
    src[T] = src[T - 1]  # last edge of tile 0 and first edge of tile 1
    with gs.Degrees("all", capacity_hint=4 * T) as D:
        _fold_dev(D, src, dst)
        tids, net = _net(src, dst, "all")
        assert net.max() == 2 and (net == 2).sum() == 1
        _check(D, tids, net)


# ------------------------------------------------------------------ deletions
def test_deletions_in_batches(gs):
    rng = np.random.default_rng(21)
    T = gs.DEGREE_TILE
    pool = rng.integers(I64_MIN, I64_MAX, size=300, dtype=np.int64)
    src, dst, dele, present = [], [], [], []
    for _ in range(2 * T + 100):
        if present and rng.random() < 0.45:  # delete an edge that is present
            s, d = present.pop(int(rng.integers(0, len(present))))
            src.append(s), dst.append(d), dele.append(1)
        else:
            s, d = int(pool[rng.integers(0, 300)]), int(pool[rng.integers(0, 300)])
            present.append((s, d))
            src.append(s), dst.append(d), dele.append(0)
    src, dst = np.array(src, np.int64), np.array(dst, np.int64)
    dele = np.array(dele, np.uint8) | 0xFE * (rng.random(len(src)) < 0.5).astype(np.uint8)  # only bit 0 is read
    for direction in DIRS:
        with gs.Degrees(direction, capacity_hint=1024) as D:
            cuts = [0, 1, 70, T + 3, len(src)]
            for a, b in zip(cuts[:-1], cuts[1:]):
                if a % 2:
                    D.fold(src[a:b], dst[a:b], dele[a:b])
                else:
                    _fold_dev(D, src[a:b], dst[a:b], dele[a:b])
                _check(D, *_net(src[:b], dst[:b], direction, dele[:b]))


def test_vertex_returns_to_zero_and_comes_back(gs):
    with gs.Degrees("all", capacity_hint=16) as D:
        D.fold([10, 10], [20, 30])
        D.fold([10], [20], [1])
        _check(D, np.array([10, 20, 30], np.int64), np.array([1, 0, 1], np.int64))
        D.fold([10], [30], [1])
        _check(D, np.array([10, 20, 30], np.int64), np.array([0, 0, 0], np.int64))
        v, d = D.degrees()
        assert len(v) == 0 and len(D.distribution()[0]) == 0
        assert D.num_vertices() == 3  # table entries, those at <= 0 included
        D.fold([20], [40])
        _check(D, np.array([10, 20, 30, 40], np.int64), np.array([0, 1, 0, 1], np.int64))


# ------------------------------------------------------------------ fold forms
def test_stride_two_and_host_fold_equal_two_arrays(gs):
    import torch
    n = gs.DEGREE_TILE + 77
    rng = np.random.default_rng(31)
    src, dst, _ = _sparse_edges(rng, n)
    dele = (rng.random(n) < 0.2).astype(np.uint8)
    for direction in DIRS:
        ids, net = _net(src, dst, direction, dele)
        with gs.Degrees(direction, capacity_hint=n) as A, gs.Degrees(direction, capacity_hint=n) as B, \
                gs.Degrees(direction, capacity_hint=n) as C:
            _fold_dev(A, src, dst, dele)
            pairs = _dev(B, np.stack([src, dst], axis=1)).contiguous().view(-1)
            te = _dev(B, dele)
            B.fold_device(pairs, pairs[1:], n=n, stride=2, deletions=te, after="torch")
            B.sync()
            C.fold(src, dst, dele)
            for X in (A, B, C):
                _check(X, ids, net)
            torch.cuda.synchronize()


# ------------------------------------------------------------------ growth, reset
def test_growth_carries_the_counts(gs):
    n = 1 << 15
    ids = (np.arange(1, 2 * n + 1, dtype=np.int64) * 2654435761) ^ 0x5555
    src, dst = np.append(ids[:n], 3), np.append(ids[n:], 4)  # 2^16 distinct endpoints and the edge (3, 4)
    first = np.zeros(n + 1, np.uint8)
    with gs.Degrees("all", capacity_hint=16) as D:
        _fold_dev(D, src, dst)
        D.fold([3], [4], [1])  # 3 and 4 stay in the table at 0
        cap1 = D.table_capacity()
        assert cap1 >= 2 * n
        second = first.copy()
        second[-1] = 1  # the second pass deletes (3, 4) once more: net -1 through the rebuild
        _fold_dev(D, src, dst, second)
        assert D.table_capacity() > cap1, "the second fold was meant to rebuild the table"
        tids = np.sort(np.concatenate([ids, [3, 4]]))
        net = np.where((tids == 3) | (tids == 4), -1, 2).astype(np.int64)
        _check(D, tids, net, absent=[5])
        assert D.num_vertices() == 2 * n + 2
        D.fold([3, 3], [4, 4])
        net[(tids == 3) | (tids == 4)] = 1
        _check(D, tids, net)


def test_reset(gs):
    rng = np.random.default_rng(41)
    src, dst, _ = _sparse_edges(rng, 1000)
    with gs.Degrees("all", capacity_hint=1000) as D:
        D.fold(src, dst)
        D.reset()
        assert D.num_vertices() == 0
        _check(D, np.zeros(0, np.int64), np.zeros(0, np.int64), absent=src[:5])
        D.fold(src[:300], dst[:300])
        _check(D, *_net(src[:300], dst[:300], "all"))


# ------------------------------------------------------------------ the sort's edges, scratch
def _distinct_ids(rng, rows):
    """`rows` distinct ids of both signs, the extremes of the key order among them."""
    special = np.array([-1, 0, I64_MIN, I64_MAX, 1, -(1 << 40)], np.int64)[:rows]
    pool = np.setdiff1d(rng.integers(I64_MIN, I64_MAX, size=2 * rows + 8, dtype=np.int64), special)
    ids = np.concatenate([special, rng.permutation(pool)[:rows - len(special)]])
    assert len(np.unique(ids)) == rows and (rows < 2 or (ids.min() < 0 <= ids.max()))
    return rng.permutation(ids)


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("rows", [1, 2047, 2048, 2049])  # one below, at, one above the sort's tile
def test_sorted_export_at_the_sort_tile(gs, rows, uniform):
    """The sorted export and the distribution at row counts around the radix sort's tile (2048
    pairs a workgroup), over ids of both signs. uniform: every vertex has degree 1, so the
    distribution's sort finds every key equal and runs no pass."""
    rng = np.random.default_rng(6000 + rows)
    ids = _distinct_ids(rng, rows)
    mult = np.ones(rows, np.int64) if uniform else 1 + (np.arange(rows) % 5) * (np.arange(rows) % 3)
    src = rng.permutation(np.repeat(ids, mult))
    dst = np.roll(src, 1)  # ("out" collects sources only)
    want_ids, want = _net(src, dst, "out")
    assert len(want_ids) == rows and np.array_equal(want_ids, np.sort(ids))
    with gs.Degrees("out", capacity_hint=rows) as D:
        _fold_dev(D, src, dst)
        _check(D, want_ids, want)
        v, d = D.degrees(sorted=True)
        assert np.array_equal(v, np.sort(ids)) and np.array_equal(d, mult[np.argsort(ids, kind="stable")])
        gd, gc_ = D.distribution()
        xd, xc = np.unique(mult, return_counts=True)
        assert np.array_equal(gd, xd) and np.array_equal(gc_, xc)
        if uniform:
            assert gd.tolist() == [1] and gc_.tolist() == [rows]


def test_scratch_is_counted_and_released(gs):
    """gs_hbm_bytes over the degree exports: each call's scratch is allocated once, kept across
    repeats and returned in full by close()."""
    import torch
    n = 5000
    src = np.arange(n, dtype=np.int64) - n // 2
    dst = src // 7 * 7
    gc.collect()  # (no summary of an earlier test is released while this one counts)
    start = gs.hbm_bytes()
    D = gs.Degrees("all", capacity_hint=n)
    try:
        assert gs.hbm_bytes() - start == gs.create_bytes("degree", n)  # no export scratch yet
        _fold_dev(D, src, dst)
        ids, net = _net(src, dst, "all")
        rows = len(ids)
        assert n <= rows <= n + 1 and D.num_vertices() == rows
        dev = torch.device("cuda", D.device)
        tv = torch.empty(rows, dtype=torch.int64, device=dev)
        td = torch.empty(rows, dtype=torch.int64, device=dev)
        held = gs.hbm_bytes()
        D.wait_stream("torch")
        assert D.degrees_device(tv, td, sorted=True) == rows
        exported = gs.hbm_bytes()
        # two (key, payload) buffers of 12 bytes a row and a 256-row histogram table, with
        # headroom, and the unordered rows (17 bytes a row of at least 0.7 x the table's slots)
        assert 2 * 12 * rows + 17 * rows <= exported - held
        k = D.distribution_device(tv, td)
        assert 0 < k < rows
        distributed = gs.hbm_bytes()
        # the CSR staging of the run heads: members, signs, heads and offsets with a quarter of headroom
        assert (8 + 1 + 16) * rows <= distributed - exported <= 2 * (8 + 1 + 16) * rows + 64
        assert D.degrees_device(tv, td, sorted=True) == rows
        assert D.distribution_device(tv, td) == k
        assert gs.hbm_bytes() == distributed
        D.degrees(sorted=True)
        D.distribution()
        host = gs.hbm_bytes()
        assert host >= distributed
        v, d = D.degrees(sorted=True)
        gd, gc_ = D.distribution()
        assert gs.hbm_bytes() == host
        assert np.array_equal(v, ids) and np.array_equal(d, net)
        xd, xc = np.unique(net, return_counts=True)
        assert np.array_equal(gd, xd) and np.array_equal(gc_, xc)
    finally:
        D.close()
    assert gs.hbm_bytes() == start


# ------------------------------------------------------------------ combine, serialize
def test_combine_and_serialize(gs):
    rng = np.random.default_rng(51)
    n = gs.DEGREE_TILE + 200
    src, dst, _ = _sparse_edges(rng, n)
    dele = np.zeros(n, np.uint8)
    dele[n // 2:] = rng.random(n - n // 2) < 0.1
    h = n // 2
    with gs.Degrees("all", capacity_hint=64) as A, gs.Degrees("all", capacity_hint=64) as B, \
            gs.Degrees("all", capacity_hint=16) as C:
        A.fold(src[:h], dst[:h], dele[:h])
        B.fold(src[h:], dst[h:], dele[h:])
        A.combine(B)
        _check(A, *_net(src, dst, "all", dele))
        _check(B, *_net(src[h:], dst[h:], "all", dele[h:]))  # the source is unchanged
        img = A.serialize()
        C.fold([1], [2])  # replaced by the image
        C.deserialize(img)
        _check(C, *_net(src, dst, "all", dele))
        assert C.num_vertices() == A.num_vertices()
        with gs.Summary("cc", capacity_hint=16) as S:
            S.fold([1, 2], [2, 3])
            with pytest.raises(gs.GSError) as e:
                S.deserialize(img)
            assert e.value.code == gs.GS_ERR_INVALID
            with pytest.raises(gs.GSError) as e:
                C.deserialize(S.serialize())
            assert e.value.code == gs.GS_ERR_INVALID
            with pytest.raises(gs.GSError) as e:
                gs._check(gs.lib().gs_combine(C.handle, S.handle))
            assert e.value.code == gs.GS_ERR_INVALID
            assert S.labels()[1].tolist() == [1, 1, 1]
        _check(C, *_net(src, dst, "all", dele))  # still works, unchanged


# ------------------------------------------------------------------ export limits
def test_truncation_and_empty(gs):
    import torch
    L = gs.lib()
    with gs.Degrees("all", capacity_hint=16) as D:
        dev = torch.device("cuda", D.device)
        got = ctypes.c_size_t(99)
        # empty: n = 0 everywhere
        v, d = D.degrees()
        assert len(v) == 0 and len(d) == 0
        assert len(D.distribution()[0]) == 0
        for fn in (L.gs_degree_export, L.gs_degree_export_device):
            got.value = 99
            assert fn(D.handle, None, None, 0, ctypes.byref(got), 1) == gs.GS_OK and got.value == 0
        for fn in (L.gs_degree_distribution, L.gs_degree_distribution_device):
            got.value = 99
            assert fn(D.handle, None, None, 0, ctypes.byref(got)) == gs.GS_OK and got.value == 0
        D.fold([1, 1, 2, 5, 1], [2, 3, 3, 5, 9])  # 1:3 2:2 3:2 5:2 9:1 -> 5 vertices, 3 distinct degrees
        tv = torch.full((4,), SENTINEL, dtype=torch.int64, device=dev)
        td = torch.full((4,), SENTINEL, dtype=torch.int64, device=dev)
        D.wait_stream("torch")
        for srt in (0, 1):
            got.value = 99
            assert L.gs_degree_export_device(D.handle, tv.data_ptr(), td.data_ptr(), 4, ctypes.byref(got),
                                             srt) == gs.GS_ERR_TRUNCATED
            assert got.value == 5
            hv = np.full(4, SENTINEL, np.int64)
            hd = np.full(4, SENTINEL, np.int64)
            got.value = 99
            assert L.gs_degree_export(D.handle, hv.ctypes.data, hd.ctypes.data, 4, ctypes.byref(got),
                                      srt) == gs.GS_ERR_TRUNCATED
            assert got.value == 5 and np.all(hv == SENTINEL) and np.all(hd == SENTINEL)
        got.value = 99
        assert L.gs_degree_distribution_device(D.handle, tv.data_ptr(), td.data_ptr(), 2,
                                               ctypes.byref(got)) == gs.GS_ERR_TRUNCATED
        assert got.value == 3
        hv = np.full(2, SENTINEL, np.int64)
        hd = np.full(2, SENTINEL, np.int64)
        got.value = 99
        assert L.gs_degree_distribution(D.handle, hv.ctypes.data, hd.ctypes.data, 2,
                                        ctypes.byref(got)) == gs.GS_ERR_TRUNCATED
        assert got.value == 3 and np.all(hv == SENTINEL) and np.all(hd == SENTINEL)
        D.sync()
        assert np.all(tv.cpu().numpy() == SENTINEL) and np.all(td.cpu().numpy() == SENTINEL)
        _check(D, np.array([1, 2, 3, 5, 9], np.int64), np.array([3, 2, 2, 2, 1], np.int64))


# ------------------------------------------------------------------ kind fences
def test_kind_fences(gs):
    import torch
    L = gs.lib()
    u64, sz, i64, ci = ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int
    a, b, c = u64(), u64(), ctypes.c_double()
    n1, n2 = sz(), sz()
    lab, fnd = i64(), ci()
    out8 = (u64 * 16)()
    grp = ctypes.c_void_p()
    gid = ctypes.create_string_buffer(gs.GROUP_ID_BYTES)
    R = ctypes.byref

    def forest_calls(h):
        return {
            "gs_fold": lambda: L.gs_fold(h, None, None, 0),
            "gs_fold_parity": lambda: L.gs_fold_parity(h, None, None, None, 0),
            "gs_fold_device": lambda: L.gs_fold_device(h, None, None, None, 0, 1),
            "gs_fold_device_after": lambda: L.gs_fold_device_after(h, None, None, None, 0, 1, None),
            "gs_fold_records_device": lambda: L.gs_fold_records_device(h, None, 0, 0),
            "gs_fold_records_counted_device": lambda: L.gs_fold_records_counted_device(h, None, 0, None, 0),
            "gs_fold_text": lambda: L.gs_fold_text(h, b"1 2\n", 4, 0, R(a), R(lab)),
            "gs_find": lambda: L.gs_find(h, 1, R(lab), R(fnd)),
            "gs_find_labels_device": lambda: L.gs_find_labels_device(h, None, 0, None, None),
            "gs_digest": lambda: L.gs_digest(h, R(a)),
            "gs_export_labels": lambda: L.gs_export_labels(h, None, None, 0, R(n1)),
            "gs_export_labels_device": lambda: L.gs_export_labels_device(h, None, None, None, 0, R(n1)),
            "gs_export_labels_part_device": lambda: L.gs_export_labels_part_device(h, 0, 1, None, None, None, 0, R(n1)),
            "gs_bip_status": lambda: L.gs_bip_status(h, R(fnd)),
            "gs_export_colouring": lambda: L.gs_export_colouring(h, None, None, None, 0, R(n1)),
            "gs_num_components": lambda: L.gs_num_components(h, R(a)),
            "gs_export_components_device": lambda: L.gs_export_components_device(h, None, None, None, None, 0, 0,
                                                                                 R(n1), R(n2)),
            "gs_export_components": lambda: L.gs_export_components(h, None, None, None, None, 0, 0, R(n1), R(n2)),
            "gs_combine_exported_device": lambda: L.gs_combine_exported_device(h, None, None, None, 0, 0),
            "gs_set_delta_tracking": lambda: L.gs_set_delta_tracking(h, 1),
            "gs_delta_capacity": lambda: L.gs_delta_capacity(h, R(a)),
            "gs_take_delta_records": lambda: L.gs_take_delta_records(h, None, 0, None),
            "gs_fold_take_device": lambda: L.gs_fold_take_device(h, None, None, 0, None, 0, None, None),
            "gs_delta_stage": lambda: L.gs_delta_stage(h, None, 0, 2, None),
            "gs_fold_exchange_device": lambda: L.gs_fold_exchange_device(h, None, None, 0, 0, 2, -1),
            "gs_set_change_tracking": lambda: L.gs_set_change_tracking(h, 1),
            "gs_take_changes_device": lambda: L.gs_take_changes_device(h, None, None, None, 0, R(a)),
            "gs_take_changes": lambda: L.gs_take_changes(h, None, None, None, 0, R(a)),
            "gs_set_window_server": lambda: L.gs_set_window_server(h, 1),
            "gs_window_server_stats": lambda: L.gs_window_server_stats(h, R(a), R(b)),
            "gs_set_pipelining": lambda: L.gs_set_pipelining(h, 2),
            "gs_set_batch_dedup": lambda: L.gs_set_batch_dedup(h, 1),
            "gs_set_profiling": lambda: L.gs_set_profiling(h, 1),
            "gs_kernel_stats": lambda: L.gs_kernel_stats(h, 0, R(a), R(c)),
            "gs_counters": lambda: L.gs_counters(h, out8),
            "gs_debug_counters": lambda: L.gs_debug_counters(h, out8, 8),
            "gs_capacity_stats": lambda: L.gs_capacity_stats(h, R(a), R(b), R(c)),
            "gs_group_create": lambda: L.gs_group_create(R(grp), h, gid, 1, 0, 1 << 16),
            "gs_group_create_partitioned": lambda: L.gs_group_create_partitioned(R(grp), h, gid, 1, 0, 1 << 10,
                                                                                 1 << 16),
        }

    def degree_calls(h):
        return {
            "gs_degree_fold": lambda: L.gs_degree_fold(h, None, None, None, 0, 0),
            "gs_degree_fold_device": lambda: L.gs_degree_fold_device(h, None, None, None, 0, 1, 0),
            "gs_degree_find_device": lambda: L.gs_degree_find_device(h, None, 0, None, None),
            "gs_degree_export_device": lambda: L.gs_degree_export_device(h, None, None, 0, R(n1), 0),
            "gs_degree_export": lambda: L.gs_degree_export(h, None, None, 0, R(n1), 1),
            "gs_degree_distribution_device": lambda: L.gs_degree_distribution_device(h, None, None, 0, R(n1)),
            "gs_degree_distribution": lambda: L.gs_degree_distribution(h, None, None, 0, R(n1)),
        }

    with gs.Degrees("all", capacity_hint=16) as D:
        D.fold([1, 2], [2, 3])
        for name, call in forest_calls(D.handle).items():
            assert call() == gs.GS_ERR_INVALID, name
            assert b"degree summary" in L.gs_last_error(), (name, L.gs_last_error())
            assert not grp.value
        # the calls every kind serves, and the handle still works
        D.sync()
        assert D.num_vertices() == 3 and D.table_capacity() >= 64 and D.stream
        st = torch.cuda.Stream(D.device)
        ev = torch.cuda.Event()
        ev.record(st)
        D.wait_stream(st)
        gs._check(L.gs_wait_event(D.handle, ev.cuda_event))
        gs._check(L.gs_reset_config(D.handle))
        assert D.num_vertices() == 0
        D.fold([1, 2], [2, 3])
        _check(D, np.array([1, 2, 3], np.int64), np.array([1, 2, 1], np.int64))
        assert gs.hbm_bytes(D.device) >= gs.create_bytes("degree", 16)
    with gs.Summary("cc", capacity_hint=16) as S:
        S.fold([1, 2], [2, 3])
        for name, call in degree_calls(S.handle).items():
            assert call() == gs.GS_ERR_INVALID, name
            assert b"not a degree summary" in L.gs_last_error(), name
        assert S.labels()[1].tolist() == [1, 1, 1]


# ------------------------------------------------------------------ overflow guard
def test_overflow_guard(gs):
    """2^10 self-loops in ALL: count 2^11 = the occurrence total; every successful combine with
    a clone doubles both exactly; the one that would pass 2^31 - 1 fails and changes nothing."""
    loop = np.full(1 << 10, 42, np.int64)
    with gs.Degrees("all", capacity_hint=16) as A, gs.Degrees("all", capacity_hint=16) as B:
        A.fold(loop, loop)
        want = 1 << 11
        failed = False
        for _ in range(24):
            B.deserialize(A.serialize())
            assert B.degrees()[1].tolist() == [want]
            rc = gs.lib().gs_combine(A.handle, B.handle)
            if 2 * want <= (1 << 31) - 1:
                assert rc == gs.GS_OK
                want *= 2
                assert A.degrees()[1].tolist() == [want] and A.degrees()[0].tolist() == [42]
            else:
                assert rc == gs.GS_ERR_CAPACITY
                assert A.degrees()[1].tolist() == [want]
                assert B.degrees()[1].tolist() == [want]
                failed = True
                break
        assert failed and want == 1 << 30
        # the refused combine left the handle usable: a fold that fits is exact
        A.fold(loop, loop)
        _check(A, np.array([42], np.int64), np.array([want + (1 << 11)], np.int64))
