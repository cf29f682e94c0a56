"""The hot index's build: which ids of a bucket it holds, from which counts (csrc/gs_hot_k.hip,
hot_after_fold in csrc/gs_capi.cpp).

The bucket stays two 8-byte keys (the 32-byte bucket of five quotiented ids was priced and not
built: profiles/hot_ways_calib.txt), so what is tested here is what changed: the sketch of one or
two rows whose smaller counter ranks an id, and the counts of k = 1, 2 or 4 folds behind one build
that takes its candidates from the last of them.

Streams have at most 2^16 edges in 2^11-edge batches. Every GPU case is exact against
oracle.cc_labels after every few batches and asserts from gs_hot_index_stats that an index
engaged; gs_testing_hot_keys says which keys it holds. Keys are put into chosen buckets with the
inverse of hot_pos's multiplier. The generators are checked without a GPU."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

I64_MIN = np.iinfo(np.int64).min
B = 1 << 11
LOG2 = 8                  # 2^8 ids: 128 buckets, chosen by the top 7 bits of key * MUL
MUL = 0xD6E8FEB86659FD93  # hot_pos's multiplier (gs_device.hpp)
INV = pow(MUL, -1, 1 << 64)
M64 = (1 << 64) - 1


def _signed(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def _product(key):
    return (int(key) * MUL) & M64


def _bucket(key, log2_ids=LOG2):
    return _product(key) >> (65 - log2_ids) if log2_ids > 1 else 0


def _key_in(top7, low):
    """The key whose product is top7 << 57 | low: in bucket top7 of 128."""
    return _signed(((top7 << 57) | low) * INV)


def _dev(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _equal(got, want, what=""):
    assert np.array_equal(got[0], want[0]), "vertex sets differ " + what
    assert np.array_equal(got[1], want[1]), "labels differ at %d vertices %s" % (int((got[1] != want[1]).sum()), what)


def _engaged(ds, log2=LOG2):
    st = ds.hot_index_stats()
    assert st["builds"] >= 1 and st["entries"] >= 1, "the hot index never engaged: %r" % (st,)
    assert st["log2_entries"] == log2 and st["entries"] <= 1 << log2
    return st


def _cold(rng, n, avoid):
    """n ids outside the buckets of `avoid`: there the named hubs are the only candidates."""
    ids = np.unique(rng.integers(-(1 << 62), 1 << 62, 4 * n, dtype=np.int64))
    ids = np.array([k for k in rng.permutation(ids) if _bucket(k) not in avoid][:n], np.int64)
    assert len(ids) == n
    return ids


def _batch(rng, hubs, counts, cold, chain=True):
    """One batch of B edges: hub i is the source of counts[i] edges to cold ids, consecutive hubs
    are joined (one component, whatever the cold sides do), and cold-cold edges fill the rest."""
    s = [np.full(c, h, np.int64) for h, c in zip(hubs, counts) if c]
    s = np.concatenate(s) if s else np.zeros(0, np.int64)
    d = cold[rng.integers(0, len(cold), len(s))]
    live = [h for h, c in zip(hubs, counts) if c]
    if chain and len(live) > 1:
        s, d = np.concatenate([s, live[:-1]]), np.concatenate([d, live[1:]])
    pad = B - len(s)
    assert pad >= 0
    s = np.concatenate([s, cold[rng.integers(0, len(cold), pad)]])
    d = np.concatenate([d, cold[rng.integers(0, len(cold), pad)]])
    p = rng.permutation(B)
    return s[p].astype(np.int64), d[p].astype(np.int64)


def _fold_checked(ds, oracle_mod, s, d, cache, check_every=2, stop=None, each=None, sizes=None):
    """Fold (s, d) in batches of B (or of `sizes`); exact labels after every check_every-th batch
    and at the end (the oracle's are computed once per stream, shared through `cache`)."""
    n = len(s) if stop is None else stop
    sizes = [B] * (n // B) if sizes is None else sizes
    assert sum(sizes) == n
    want = cache.setdefault("want", {})
    ts, td = _dev(s, d)
    o = 0
    for k, c in enumerate(sizes):
        ds.fold_device(ts[o:], td[o:], n=c)
        o += c
        if each:
            each(k)
        if (k + 1) % check_every == 0 or o == n:
            if o not in want:
                want[o] = oracle_mod.cc_labels(s[:o], d[:o])
            _equal(ds.labels(), want[o], "after %d edges" % o)


# ---- 1. overfull and underfull buckets: the two most frequent hubs of a bucket are held ----

_FULL = {}
_FULL_BUCKETS = {0x11: 1, 0x22: 2, 0x33: 3, 0x44: 5}   # bucket: hubs in it, of frequencies 2^(8 - i) per batch


def _overfull():
    if "s" not in _FULL:
        rng = np.random.default_rng(0x5A1)
        hubs, counts, expect = [], [], set()
        for top, m in _FULL_BUCKETS.items():
            ks = [_key_in(top, 1 + 977 * i) for i in range(m)]
            hubs += ks
            counts += [256 >> i for i in range(m)]
            expect |= set(ks[:2])
        cold = _cold(rng, 800, set(_FULL_BUCKETS))
        bs = [_batch(rng, hubs, counts, cold) for _ in range(8)]
        _FULL.update(s=np.concatenate([b[0] for b in bs]), d=np.concatenate([b[1] for b in bs]),
                     hubs=np.array(hubs, np.int64), expect=expect)
    return _FULL["s"], _FULL["d"], _FULL["hubs"], _FULL["expect"]


def test_generators_reach_their_buckets():
    s, d, hubs, expect = _overfull()
    per = {}
    for k in hubs:
        per.setdefault(_bucket(k), []).append(int(k))
    assert {b: len(v) for b, v in per.items()} == _FULL_BUCKETS
    ends = np.concatenate([s[:B], d[:B]])
    for b, ks in per.items():
        cnt = [int((ends == k).sum()) for k in ks]
        assert all(x >= 2 * y - 4 for x, y in zip(cnt, cnt[1:])), cnt   # far apart, in the listed order
        assert set(ks[:2]) <= expect
    others = np.setdiff1d(ends, hubs)
    assert not {_bucket(k) for k in others} & set(_FULL_BUCKETS)       # the hubs are alone in their buckets
    for k in (1, 2, 4):
        s, d, a, b, c, z = _sample_stream(k)
        assert len({_bucket(x) for x in (a, b, c, z)}) == 1
        last = 3 + k - 1
        ends = np.concatenate([s[last * B:(last + 1) * B], d[last * B:(last + 1) * B]])
        assert z not in ends and all(x in ends for x in (a, b, c))
    pairs = _alias_pairs()
    for (x, y), bit in zip(pairs, (0, 50, 51)):
        assert _product(x) ^ _product(y) == 1 << bit
    assert all(_bucket(x) == _bucket(y) for x, y in pairs)             # each pair shares a bucket of 128
    assert _bucket(pairs[2][0], 16) != _bucket(pairs[2][1], 16)        # (not of 2^15)


@gpu
@pytest.mark.parametrize("sketch_log2", [0, 5])
@pytest.mark.parametrize("rows", [1, 2])
def test_the_two_most_frequent_hubs_of_a_bucket_are_held(gs, oracle_mod, rows, sketch_log2):
    """Buckets that receive 1, 2, 3 and 5 hubs whose frequencies are a factor 2 apart: whatever the
    sketch (one row or two; one counter per id, where every counter is shared, or 32), the two
    most frequent of each are held and no other. A shared counter only adds the sharers' counts:
    with one counter per id (2^8 counters for 811 ids) a hub's count is overstated by its
    counter's cold ids, some 3 ids of about 5 occurrences each: far less than the 64 between the
    second and the third hub of a bucket."""
    s, d, hubs, expect = _overfull()
    with gs.Summary("cc", capacity_hint=1 << 12) as ds:
        ds.set_hot_index(LOG2, 0, 1000000)
        gs.testing_hot_tune(ds, rows=rows, sketch_log2=sketch_log2)

        def each(k):
            if k == 0:
                assert _engaged(ds)["builds"] == 1
                held = set(gs.testing_hot_keys(ds).tolist())
                assert held & set(hubs.tolist()) == expect

        _fold_checked(ds, oracle_mod, s, d, _FULL, each=each)
        assert _engaged(ds)["builds"] == 1


# ---- 2. keys whose products nearly alias, and the ids that are never held ----

_ALIAS = {}


def _alias_pairs():
    p = (0x5B << 57) | 0x0123456789ABCDE
    return [(_signed(p * INV), _signed((p ^ 1) * INV)),                 # products that differ in bit 0 only
            (_signed((p + 4) * INV), _signed(((p + 4) ^ (1 << 50)) * INV)),   # ... in bit 50 only
            (_signed((p + 8) * INV), _signed(((p + 8) ^ (1 << 51)) * INV))]   # ... in bit 51 only


def _aliasing():
    if "s" not in _ALIAS:
        rng = np.random.default_rng(0x5A2)
        pairs = _alias_pairs()
        zero_low = _key_in(0x2D, 0)            # a product whose low 51 bits are 0
        hubs = [k for pr in pairs for k in pr] + [zero_low, I64_MIN]
        cold = _cold(rng, 600, {_bucket(k) for k in hubs})
        bs = []
        for j in range(8):
            # each pair's first key is tied to one half of the cold ids, its second to the other:
            # keys taken for one another would join the halves
            s, d = [], []
            for i, (x, y) in enumerate(pairs):
                m = 96 - 16 * i
                s += [x] * m + [y] * m
                d += list(cold[rng.integers(0, 300, m)]) + list(cold[300 + rng.integers(0, 300, m)])
            s += [I64_MIN] * 300 + [zero_low] * 200
            d += list(cold[rng.integers(0, 300, 500)])
            if j >= 6:   # late: the halves are joined through one pair
                s.append(pairs[1][0])
                d.append(pairs[1][1])
            pad = B - len(s)
            lo = rng.integers(0, 2, pad) * 300
            s += list(cold[lo + rng.integers(0, 300, pad)])
            d += list(cold[lo + rng.integers(0, 300, pad)])
            p = rng.permutation(B)
            bs.append((np.array(s, np.int64)[p], np.array(d, np.int64)[p]))
        _ALIAS.update(s=np.concatenate([b[0] for b in bs]), d=np.concatenate([b[1] for b in bs]), zero_low=zero_low)
    return _ALIAS["s"], _ALIAS["d"], _ALIAS["zero_low"]


@gpu
@pytest.mark.parametrize("rows", [1, 2])
def test_keys_whose_products_nearly_alias(gs, oracle_mod, rows):
    """Pairs of frequent keys whose products differ in bit 0, bit 50 or bit 51 only, each key of a
    pair in another component until a late edge joins them; INT64_MIN as the most frequent endpoint
    is never held, and a key whose product's low 51 bits are 0 is an id like any other."""
    s, d, zero_low = _aliasing()
    with gs.Summary("cc", capacity_hint=1 << 12) as ds:
        ds.set_pipelining(2)
        ds.set_hot_index(LOG2, 0, 2)
        gs.testing_hot_tune(ds, rows=rows)

        def each(k):
            if k % 2 == 1:
                assert I64_MIN not in gs.testing_hot_keys(ds).tolist()

        _fold_checked(ds, oracle_mod, s, d, _ALIAS, check_every=1, each=each)
        assert _engaged(ds)["builds"] >= 2


# ---- 3. counts over k folds, candidates from the last ----

_SAMPLE = {}
_X = 0x66   # the bucket of a, b, c and z


def _sample_stream(k):
    """Folds 0-2 and the k - 1 folds after them are `rich`: c 100 times, z 200 times, a 8, b 6. From
    fold 3 + k - 1 on: a 8, b 6, c 4, and no z. With first_after_edges = 3 B + 1 a build is due
    from fold 3 on: it follows fold 3 + k - 1, the first without z, and counts the k - 1 rich folds
    before it too."""
    if k not in _SAMPLE:
        rng = np.random.default_rng(0x5A3 + k)
        a, b, c, z = (_key_in(_X, low) for low in (3, 5, 7, 11))
        far = [_key_in(0x07 + 9 * i, 13) for i in range(6)]   # hubs elsewhere: the giant the index serves
        cold = _cold(rng, 700, {_X})
        hubs = [a, b, c, z] + far
        rich, last = [8, 6, 100, 200] + [120] * 6, [8, 6, 4, 0] + [120] * 6
        bs = [_batch(rng, hubs, rich if j < 3 + k - 1 else last, cold) for j in range(10)]
        _SAMPLE[k] = dict(s=np.concatenate([x[0] for x in bs]), d=np.concatenate([x[1] for x in bs]), keys=(a, b, c, z))
    c_ = _SAMPLE[k]
    return (c_["s"], c_["d"]) + c_["keys"]


@gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_counts_of_k_folds_candidates_from_the_last(gs, oracle_mod, k, depth):
    """The hot ids change between the counted folds. z, the most frequent id of the counted folds
    before the last, is not in the last: never a candidate. One fold's counts hold a and b; with
    the folds before, c (100 (k - 1) + 4 occurrences against a's 8 k) takes the first place."""
    s, d, a, b, c, z = _sample_stream(k)
    build_fold = 3 + k - 1
    with gs.Summary("cc", capacity_hint=1 << 12) as ds:
        ds.set_pipelining(depth)
        ds.set_hot_index(LOG2, 3 * B + 1, 1000000)
        gs.testing_hot_tune(ds, sample_folds=k)

        def each(i):
            if i == build_fold - 1:
                assert ds.hot_index_stats()["builds"] == 0   # folds 3 .. 3 + k - 2 are only counted
            if i == build_fold:
                assert _engaged(ds)["builds"] == 1
                held = set(gs.testing_hot_keys(ds).tolist()) & {a, b, c, z}
                assert held == ({a, b} if k == 1 else {c, a})

        _fold_checked(ds, oracle_mod, s, d, _SAMPLE[k], each=each)
        assert _engaged(ds)["builds"] == 1


@gpu
@pytest.mark.parametrize("how", ["reset", "regrow"])
def test_a_partly_counted_sketch_is_discarded(gs, oracle_mod, how):
    """k = 4. Two rich folds are counted (c 100 times each); then the table's life ends, by a reset
    or by a regrow (one fold of 2^14 edges between 2^15 new ids: more than the table holds). No
    build comes from the stale sketch: the next one follows the fourth fold of the new life, and
    its counts (a above b above c, a few dozen each) hold a and b. With the stale counts it would
    have come two folds earlier and held c."""
    s, d, a, b, c, z = _sample_stream(1)           # folds 0-2 rich, the others not
    big, sizes, first = 1 << 14, None, 2
    if how == "regrow":                            # the regrowing fold is the new life's first
        fresh = _cold(np.random.default_rng(0x5A7), 2 * big, {_X})
        s = np.concatenate([s[:2 * B], fresh[:big], s[3 * B:]])
        d = np.concatenate([d[:2 * B], fresh[big:], d[3 * B:]])
        sizes = [B, B, big] + [B] * 7
    with gs.Summary("cc", capacity_hint=1 << 12) as ds:
        ds.set_pipelining(2)
        ds.set_hot_index(LOG2, 0, 1000000)
        gs.testing_hot_tune(ds, sample_folds=4)
        if how == "reset":
            _fold_checked(ds, oracle_mod, s, d, {}, stop=2 * B)
            assert ds.hot_index_stats()["builds"] == 0
            ds.reset()
            s, d, first = s[3 * B:], d[3 * B:], 0
        seen = {}

        def each(i):
            if how == "regrow" and i == 1:
                seen["cap"] = ds.table_capacity()
                assert ds.hot_index_stats()["builds"] == 0
            if how == "regrow" and i == 2:
                assert ds.table_capacity() > seen["cap"], "the table was to grow in this fold"
            if i == first + 2:
                assert ds.hot_index_stats()["builds"] == 0
            if i == first + 3:
                assert _engaged(ds)["builds"] == 1
                assert set(gs.testing_hot_keys(ds).tolist()) & {a, b, c, z} == {a, b}
                seen["built"] = True

        _fold_checked(ds, oracle_mod, s, d, {}, each=each, sizes=sizes)
        assert seen.get("built") and _engaged(ds)["builds"] == 1
