"""GPU: the hot index of the plain CC fold (gs_set_hot_index, csrc/gs_hot_k.hip).

An index entry may only settle an edge whose endpoints it places under one ancestor, so every
result must stay what the oracle computes: all comparisons are exact equality of the
(vertex, label) arrays. Every test that forces an index on also asserts from
gs_hot_index_stats that a build ran and placed entries -- a run in which the index silently
stayed off must not pass.

Shapes: ids from a pool of 4096 in 64 communities with a hub each (a hub is an endpoint of
about every second edge of its community, and the communities' sizes are skewed), 2^16 edges in
2^11-edge batches: 8 blocks per fold, a few dozen ids above every index size used here (2^1 ..
2^8 entries), so positions collide, hubs are evicted and most edges have one or no endpoint in
the index. A few edges between communities keep merging hub components after the index was
built (stale ancestors)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
N, B = 1 << 16, 1 << 11


def _stream(seed, n=N, pool=4096, comms=64, cross=0.002):
    rng = np.random.default_rng(seed)
    ids = np.unique(rng.integers(-(1 << 62), 1 << 62, 2 * pool, dtype=np.int64))[:pool]
    ids = rng.permutation(ids)
    per = pool // comms
    w = 1.0 / np.arange(1, comms + 1)
    c = rng.choice(comms, n, p=w / w.sum())

    def side(c, hub_p):
        m = rng.integers(0, per, n)
        m[rng.random(n) < hub_p] = 0
        return ids[c * per + m]

    c2 = c.copy()
    x = rng.random(n) < cross
    c2[x] = rng.integers(0, comms, int(x.sum()))
    return side(c, 0.5), side(c2, 0.3)


_CACHE = {}


def _case(oracle_mod):
    """The skewed stream and its oracle labels after every 4th batch, computed once."""
    if "case" not in _CACHE:
        s, d = _stream(0x407)
        marks = list(range(4 * B, N + 1, 4 * B))
        _CACHE["case"] = (s, d, {m: oracle_mod.cc_labels(s[:m], d[:m]) for m in marks})
    return _CACHE["case"]


def _engaged(ds, log2=None):
    st = ds.hot_index_stats()
    assert st["builds"] >= 1 and st["entries"] >= 1, "the hot index never engaged: %r" % (st,)
    if log2 is not None:
        assert st["log2_entries"] == log2
    return st


def _equal(got, want, what=""):
    assert np.array_equal(got[0], want[0]), "vertex sets differ " + what
    assert np.array_equal(got[1], want[1]), "labels differ at %d vertices %s" % (int((got[1] != want[1]).sum()), what)


def _fold_all(ds, ts, td, n=None, b=B, each=None):
    n = ts.numel() if n is None else n
    for k, o in enumerate(range(0, n, b)):
        ds.fold_device(ts[o:], td[o:], n=min(b, n - o))
        if each:
            each(k, o + min(b, n - o))


def _dev(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _off_labels(gs, depth, oracle_mod):
    """Labels of the same run with the index off, per pipelining depth (computed once)."""
    key = ("off", depth)
    if key not in _CACHE:
        s, d, _ = _case(oracle_mod)
        ts, td = _dev(s, d)
        with gs.Summary("cc", capacity_hint=1 << 14) as ds:
            ds.set_pipelining(depth)
            ds.set_hot_index(-1)
            _fold_all(ds, ts, td)
            _CACHE[key] = ds.labels()
            assert ds.hot_index_stats()["builds"] == 0
    return _CACHE[key]


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("every", [1, 3, 32])
@pytest.mark.parametrize("log2", [4, 6, 8])
def test_skewed_stream(gs, oracle_mod, log2, every, depth):
    """every = 32: one build, then a refresh of the entries' ancestors every second fold."""
    s, d, want = _case(oracle_mod)
    ts, td = _dev(s, d)
    with gs.Summary("cc", capacity_hint=1 << 14) as ds:
        cap0 = ds.table_capacity()
        ds.set_pipelining(depth)
        ds.set_hot_index(log2, 0, every)

        def each(k, done):
            if (k + 1) % 4 == 0:
                _equal(ds.labels(), want[done], "after %d edges" % done)

        _fold_all(ds, ts, td, each=each)
        got = ds.labels()
        _equal(got, want[N], "at the end")
        _equal(got, _off_labels(gs, depth, oracle_mod), "against the run with the index off")
        st = _engaged(ds, log2)
        if every < 16:
            assert st["builds"] >= 2 and st["refreshes"] == 0  # rebuilt along the way
        else:
            assert st["refreshes"] >= 2  # (a refresh is queued only once the last one was adopted)
        assert ds.table_capacity() == cap0  # one life of the table: the index was never dropped by a rebuild


def test_stale_ancestor(gs, oracle_mod):
    """A hub's entry names the hub's root of build time; the component is then hooked under a
    smaller id and the hub goes on receiving edges: the final labels carry the smaller id."""
    hub, low = 1000, 5
    a = np.arange(2000, 3000, dtype=np.int64)
    b = np.arange(3000, 4000, dtype=np.int64)
    parts = [(np.full(1000, hub, np.int64), a),                       # the hub's component (label 1000)
             (np.array([hub, 7777], np.int64), np.array([hub, 7777], np.int64)),  # (a fold that adopts the build)
             (np.array([low], np.int64), np.array([2500], np.int64)),  # hooks it under 5
             (b, np.full(1000, hub, np.int64)),                        # more edges on the hub
             (np.full(500, hub, np.int64), a[:500])]
    with gs.Summary("cc", capacity_hint=1 << 12) as ds:
        ds.set_hot_index(6, 0, 1000000)  # one build, after the first fold
        for i, (s, d) in enumerate(parts):
            ds.fold(s, d)
            if i == 0:
                st = _engaged(ds, 6)
                assert st["builds"] == 1
        assert ds.hot_index_stats()["builds"] == 1  # the stale index served every later fold
        s = np.concatenate([p[0] for p in parts])
        d = np.concatenate([p[1] for p in parts])
        got = ds.labels()
        _equal(got, oracle_mod.cc_labels(s, d))
        assert got[1][got[0] == hub][0] == low and got[1][got[0] == 3999][0] == low


def test_table_rebuild_with_live_index(gs, oracle_mod):
    s, d, want = _case(oracle_mod)
    ts, td = _dev(s, d)
    with gs.Summary("cc", capacity_hint=64) as ds:
        cap0 = ds.table_capacity()
        ds.set_hot_index(6, 0, 1)
        grown_live = []

        def each(k, done):
            if (k + 1) % 4 == 0:
                grown_live.append((ds.table_capacity(), ds.hot_index_stats()["entries"]))
                _equal(ds.labels(), want[done], "after %d edges" % done)

        _fold_all(ds, ts, td, each=each)
        _equal(ds.labels(), want[N])
        _engaged(ds, 6)
        assert ds.table_capacity() > cap0, "the table was to be rebuilt during the run"
        assert any(c > cap0 and e >= 1 for c, e in grown_live)  # an index was live again after a rebuild


def test_reset_between_two_passes(gs, oracle_mod):
    s, d, want = _case(oracle_mod)
    rng = np.random.default_rng(11)
    s2, d2 = rng.permutation(s)[: N // 2], rng.permutation(d)[: N // 2]  # another stream over the same ids
    ts, td, ts2, td2 = _dev(s, d, s2, d2)
    with gs.Summary("cc", capacity_hint=1 << 14) as ds:
        ds.set_pipelining(3)
        ds.set_hot_index(8, 0, 2)
        _fold_all(ds, ts, td)
        _equal(ds.labels(), want[N])
        b1 = _engaged(ds, 8)["builds"]
        ds.reset()
        assert ds.hot_index_stats()["log2_entries"] == 0  # dropped with the table's life
        _fold_all(ds, ts2, td2)
        _equal(ds.labels(), oracle_mod.cc_labels(s2, d2), "after the reset")
        assert _engaged(ds, 8)["builds"] > b1


@pytest.mark.parametrize("log2", [1, 4])
def test_special_ids_and_small_index(gs, oracle_mod, log2):
    """INT64_MIN (the table's empty marker, kept in the reserved slot), INT64_MAX and -1 (the
    key an empty index entry carries) as the most frequent ids; self-loops on hot ids; edges with
    both, one and no endpoint in the index. log2 = 1: two entries, every hot id collides."""
    rng = np.random.default_rng(5)
    hot = np.array([I64_MIN, I64_MAX, -1, 0, 42], np.int64)
    cold = rng.integers(-(1 << 50), 1 << 50, 600, dtype=np.int64)
    n = 1 << 13
    kind = rng.integers(0, 5, n)
    h1, h2 = hot[rng.integers(0, 5, n)], hot[rng.integers(0, 3, n) + 2]
    c1, c2 = cold[rng.integers(0, 600, n)], cold[rng.integers(0, 600, n)]
    s = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [h2, h2, h2, c1], c1)
    d = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [h2, s, c2[:n] | 1, h2], c2)
    lo = rng.integers(0, 2, n)
    m = rng.random(n) < 0.25  # INT64_MIN / INT64_MAX: self-loops, each other, and cold even ids
    s[m] = hot[lo[m]]
    d[m] = np.where(rng.random(int(m.sum())) < 0.5, hot[rng.integers(0, 2, int(m.sum()))], c1[m] & ~np.int64(1))
    s[-3:] = [I64_MIN, I64_MAX, -1]
    d[-3:] = [-1, 42, I64_MIN]
    ts, td = _dev(s, d)
    with gs.Summary("cc", capacity_hint=1 << 12) as ds:
        ds.set_pipelining(2)
        ds.set_hot_index(log2, 0, 1)
        b = 1 << 10
        _fold_all(ds, ts, td, b=b, each=lambda k, done: k == 3 and _equal(
            ds.labels(), oracle_mod.cc_labels(s[:done], d[:done]), "after %d edges" % done))
        _equal(ds.labels(), oracle_mod.cc_labels(s, d))
        st = _engaged(ds, log2)
        assert st["entries"] <= 1 << log2


def test_doors_between_folds(gs, oracle_mod):
    import torch
    s, d, want = _case(oracle_mod)
    ts, td = _dev(s, d)
    o_s = np.array([1, 2, 3], np.int64)
    o_d = np.array([2, 3, int(s[0])], np.int64)  # the other summary's component reaches into this one
    q = torch.from_numpy(np.concatenate([np.unique(s)[:512], [123456789]])).cuda()
    lab = torch.empty_like(q)
    found = torch.empty(q.numel(), dtype=torch.uint8, device="cuda")
    with gs.Summary("cc", capacity_hint=1 << 14) as ds, gs.Summary("cc", capacity_hint=16) as other:
        other.fold(o_s, o_d)
        ds.set_pipelining(3)
        ds.set_hot_index(6, 0, 2)
        half = N // 2

        def each(k, done):
            if k == 5:
                ds.find_labels_device(q, lab, found)
                ds.sync()
            if k == 9:
                assert ds.num_components() == len(set(oracle_mod.cc_labels(s[:done], d[:done])[1].tolist()))
            if done == half:
                _equal(ds.labels(), want[half])
                _engaged(ds, 6)
                ds.combine(other)
                assert ds.hot_index_stats()["log2_entries"] == 0  # the combine dropped the index

        _fold_all(ds, ts, td, each=each)
        allv = oracle_mod.cc_labels(np.concatenate([s, o_s]), np.concatenate([d, o_d]))
        _equal(ds.labels(), allv, "after the combine")
        _engaged(ds, 6)
        ds.find_labels_device(q, lab, found)
        ds.sync()
        look = dict(zip(allv[0].tolist(), allv[1].tolist()))
        hq, hl, hf = q.cpu().numpy(), lab.cpu().numpy(), found.cpu().numpy()
        assert hf[-1] == 0 and hf[:-1].all()
        assert [look[v] for v in hq[:-1].tolist()] == hl[:-1].tolist()


def test_refused_kinds(gs):
    with gs.Summary("signed", capacity_hint=64) as c:
        with pytest.raises(gs.GSError) as e:
            c.set_hot_index(4, 0, 1)
        assert e.value.code == gs.GS_ERR_INVALID
    with gs.Degrees(capacity_hint=64) as g:
        assert gs.lib().gs_set_hot_index(g._h, 4, 0, 1) == gs.GS_ERR_INVALID


def test_tracked_and_take_folds_untouched(gs, oracle_mod):
    import torch
    s, d, want = _case(oracle_mod)
    ts, td = _dev(s, d)
    rec = torch.empty((B, 3), dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n = N // 4
    with gs.Summary("cc", capacity_hint=1 << 14) as tr, gs.Summary("cc", capacity_hint=1 << 14) as tk:
        for x in (tr, tk):
            x.set_hot_index(6, 0, 1)
            x.set_delta_tracking(True)
        for o in range(0, n, B):
            tr.fold_device(ts[o:], td[o:], n=B)
            tr.take_delta_records(rec, B, cnt)
            tr.sync()
            k = tk.fold_take(ts[o:], td[o:], B, rec, B, cnt)
            assert 0 <= k <= B
        for x in (tr, tk):
            _equal(x.labels(), want[n])
            assert x.hot_index_stats()["builds"] == 0  # never active in tracked or take folds


def test_group_folds_untouched(gs, oracle_mod):
    s, d, want = _case(oracle_mod)
    ts, td = _dev(s, d)
    n = N // 4
    with gs.Summary("cc", capacity_hint=1 << 14) as x:
        x.set_hot_index(6, 0, 1)
        g = gs.Group(x, gs.group_unique_id(), 1, 0, B)
        for o in range(0, n, B):
            g.fold_device(ts[o:], td[o:], B)
        g.finish()
        got = x.labels()
        builds = x.hot_index_stats()["builds"]
        g.close()
    _equal(got, want[n])
    assert builds == 0
