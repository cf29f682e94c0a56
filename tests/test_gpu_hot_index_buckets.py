"""GPU: the hot index's two-key buckets and single ancestor (csrc/gs_hot_k.hip, fold_block<..., HOT>).

A bucket holds two keys and nothing else; a key is held only if its slot is under the build's
ancestor G, and the header beside the buckets carries G and a root G2 found from it later. Two
hits settle an edge, one hit settles it when the other side's first probe is, or hangs directly
under, G or G2. The results must stay what the oracle computes: every comparison is exact equality
of the (vertex, label) arrays, and every case that forces an index on asserts from
gs_hot_index_stats that a build ran and holds keys.

Shapes as in test_gpu_hot_index.py: at most 2^16 edges in 2^11-edge batches (8 blocks per fold),
ids from a pool of 4096, index sizes 2^1 .. 2^8 ids (one bucket .. 128 buckets)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
B = 1 << 11
MUL = 0xD6E8FEB86659FD93  # hot_pos's multiplier (gs_device.hpp)
INV = pow(MUL, -1, 1 << 64)


def _signed(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _bucket(key, log2_ids):
    """hot_pos: the bucket of a key in an index of 2^log2_ids ids."""
    return ((key * MUL) & ((1 << 64) - 1)) >> (65 - log2_ids) if log2_ids > 1 else 0


def _key_in(top7, low):
    """The key whose hash starts with the 7 bits top7: one bucket at every size up to 2^8 ids."""
    return _signed(((top7 << 57) | low) * INV)


def _dev(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _equal(got, want, what=""):
    assert np.array_equal(got[0], want[0]), "vertex sets differ " + what
    assert np.array_equal(got[1], want[1]), "labels differ at %d vertices %s" % (int((got[1] != want[1]).sum()), what)


def _engaged(ds, log2):
    st = ds.hot_index_stats()
    assert st["builds"] >= 1 and st["entries"] >= 1, "the hot index never engaged: %r" % (st,)
    assert st["log2_entries"] == log2 and st["entries"] <= 1 << log2
    return st


def _run(gs, oracle_mod, s, d, log2, every, cache, hint=1 << 14, check_every=4, depth=1):
    """Fold (s, d) in batches of B; the oracle's labels after every check_every-th batch and at the
    end (computed once per stream, shared through `cache`)."""
    n = len(s)
    if "want" not in cache:
        marks = sorted(set(list(range(check_every * B, n + 1, check_every * B)) + [n]))
        cache["want"] = {m: oracle_mod.cc_labels(s[:m], d[:m]) for m in marks}
    want = cache["want"]
    ts, td = _dev(s, d)
    with gs.Summary("cc", capacity_hint=hint) as ds:
        cap0 = ds.table_capacity()
        ds.set_pipelining(depth)
        ds.set_hot_index(log2, 0, every)
        for o in range(0, n, B):
            c = min(B, n - o)
            ds.fold_device(ts[o:], td[o:], n=c)
            if o + c in want:
                _equal(ds.labels(), want[o + c], "after %d edges" % (o + c))
        st = _engaged(ds, log2)
        assert ds.table_capacity() == cap0  # one life of the table
        return st


def _pool(seed, n=4096):
    rng = np.random.default_rng(seed)
    ids = np.unique(rng.integers(-(1 << 62), 1 << 62, 2 * n, dtype=np.int64))[:n]
    return rng, rng.permutation(ids)


# ---- 1. two large components, hubs in each; then edges between their hubs ----

_TWO = {}


def _two_components():
    if "s" not in _TWO:
        rng, ids = _pool(0x2C0)
        half = len(ids) // 2
        n, n1 = 1 << 16, 1 << 15
        side = rng.integers(0, 2, n)                       # the edge's component
        hub = ids[side * half + rng.integers(0, 4, n)]     # 4 hubs each, equally frequent
        mem = ids[side * half + rng.integers(0, half, n)]
        mem2 = ids[side * half + rng.integers(0, half, n)]
        s = np.where(rng.random(n) < 0.7, hub, mem2)
        d = mem.copy()
        # after the first half: a few edges between hubs of the two components (both frequent ids:
        # an index that held hubs of both and settled on two hits would lose this union)
        x = np.flatnonzero((np.arange(n) >= n1 + 5) & (rng.random(n) < 0.003))
        s[x] = ids[rng.integers(0, 4, len(x))]
        d[x] = ids[half + rng.integers(0, 4, len(x))]
        _TWO["s"], _TWO["d"], _TWO["x0"], _TWO["hubs"] = s, d, int(x[0]), (ids[0], ids[half])
    return _TWO["s"], _TWO["d"], _TWO["x0"]


@pytest.mark.parametrize("every", [4, 1000000])
@pytest.mark.parametrize("log2", [1, 4, 8])
def test_two_components_merge_through_their_hubs(gs, oracle_mod, log2, every):
    s, d, x0 = _two_components()
    _run(gs, oracle_mod, s, d, log2, every, _TWO)
    want = _TWO["want"]
    before, after = want[(x0 // (4 * B)) * 4 * B], want[len(s)]
    ha, hb = _TWO["hubs"]
    lab = lambda w, v: int(w[1][w[0] == v][0])
    assert lab(before, ha) != lab(before, hb) and lab(after, ha) == lab(after, hb)  # the stream does what it says


# ---- 2. the giant's root changes after the build ----

_ROOT = {}


def _root_change():
    """Batches: 0-3 a giant component around 4 hubs (the build follows batch 0); 4 a new minimum id
    hooks the giant; 5-11 hub-cold edges whose cold side hangs under the old root (members from
    before), under the new root (vertices first tied to the new minimum), is a root itself (seen
    only through a self-loop so far, or in a component of its own), or is new to the table."""
    if "s" not in _ROOT:
        rng, ids = _pool(0x2C1)
        ids = np.sort(ids)
        low, ids = ids[0], rng.permutation(ids[1:])
        hubs, old, fresh, lone, unseen = ids[:4], ids[4:2000], ids[2000:2600], ids[2600:3200], ids[3200:3800]
        ss, dd = [], []

        def batch(s, d):
            pad = B - len(s)
            assert pad >= 0
            ss.append(np.concatenate([s, hubs[rng.integers(0, 4, pad)]]))
            dd.append(np.concatenate([d, old[rng.integers(0, len(old), pad)]]))

        for _ in range(4):
            batch(hubs[rng.integers(0, 4, B)], old[rng.integers(0, len(old), B)])
        batch(np.array([low]), old[:1])                                    # the new minimum: the root changes
        for k in range(7):
            f, l, u = fresh[k::7], lone[k::7], unseen[k::7]
            h = lambda m: hubs[rng.integers(0, 4, m)]
            s = np.concatenate([np.full(len(f), low), l[::2], l[1::2][:-1]])  # under the new root; self-loops; a chain
            d = np.concatenate([f, l[::2], l[1::2][1:]])
            batch(s, d)
            s = np.concatenate([h(len(f)), l, h(len(u)), h(300)])          # hub-cold edges of every kind
            d = np.concatenate([f, h(len(l)), u, old[rng.integers(0, len(old), 300)]])
            p = rng.permutation(len(s))
            batch(s[p], d[p])
        _ROOT["s"], _ROOT["d"], _ROOT["low"] = np.concatenate(ss), np.concatenate(dd), low
    return _ROOT["s"], _ROOT["d"], _ROOT["low"]


@pytest.mark.parametrize("every", [32, 1000000])
@pytest.mark.parametrize("log2", [2, 6])
def test_root_change_after_the_build(gs, oracle_mod, log2, every):
    s, d, low = _root_change()
    st = _run(gs, oracle_mod, s, d, log2, every, _ROOT, check_every=1)
    if every == 32:
        assert st["builds"] == 1 and st["refreshes"] >= 2   # a refresh every second fold
    else:
        assert st["builds"] == 1 and st["refreshes"] == 0   # the header's G2 stays the root of build time
    want = _ROOT["want"][len(s)]
    assert want[1].min() == low and (want[1] == low).sum() > 3000


# ---- 3. keys that share a bucket, and the special ids ----

_SHARE = {}


def _sharing():
    if "s" not in _SHARE:
        rng, ids = _pool(0x2C2)
        a = [_key_in(0x55, low) for low in (1, 2, 3, 0x123456789, 1 << 56)]   # five keys of one bucket
        b = [_key_in(0x2A, low) for low in (7, 8, 9)]                        # three of another
        for log2 in range(1, 9):
            assert len({_bucket(k, log2) for k in a}) == 1 and len({_bucket(k, log2) for k in b}) == 1
        assert _bucket(a[0], 8) != _bucket(b[0], 8)
        one_bit = [a[0] ^ 1, a[0] ^ (1 << 40), _signed(a[1] ^ (1 << 63)), 1 << 40, -1 ^ (1 << 40)]
        special = [I64_MAX, -1, 0, I64_MIN + 1, I64_MIN]
        hubs = np.array(a + b + one_bit + special, np.int64)
        w = 1.0 / np.arange(1, len(hubs) + 1) ** 0.7          # distinct frequencies: a strict order in every bucket
        w[-1] = w[0]                                          # INT64_MIN is among the most frequent endpoints
        n = 1 << 14
        h1 = hubs[rng.choice(len(hubs), n, p=w / w.sum())]
        h2 = hubs[rng.choice(len(hubs), n, p=w / w.sum())]
        cold = ids[rng.integers(0, 800, n)]
        kind = rng.integers(0, 8, n)
        s = np.select([kind < 4, kind == 4, kind == 5, kind == 6], [h1, h1, h1, cold], cold)
        d = np.select([kind < 4, kind == 4, kind == 5, kind == 6], [cold, h2, h1, h2], ids[rng.integers(0, 800, n)])
        _SHARE["s"], _SHARE["d"], _SHARE["hubs"] = s, d, hubs
    return _SHARE["s"], _SHARE["d"], _SHARE["hubs"]


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("log2", [1, 2, 4, 8])
def test_keys_sharing_a_bucket_and_special_ids(gs, oracle_mod, log2, every):
    """Five and three keys in one bucket each (the weakest are evicted), keys one bit apart,
    INT64_MAX, -1, 0, INT64_MIN + 1 as frequent ids, and INT64_MIN (the reserved slot: never held,
    never a hit) as one of the most frequent endpoints."""
    s, d, hubs = _sharing()
    st = _run(gs, oracle_mod, s, d, log2, every, _SHARE, hint=1 << 12, check_every=2, depth=2)
    assert st["builds"] >= 2
    if log2 == 1:
        assert st["entries"] <= 2


# ---- 4. duplicates, self-loops, and an id the table does not hold at build time ----

_DUP = {}


def _duplicates():
    if "s" not in _DUP:
        rng, ids = _pool(0x2C3)
        hubs, late, cold = ids[:3], ids[3:5], ids[5:1500]
        n = 1 << 14
        kind = rng.integers(0, 6, n)
        h = hubs[rng.integers(0, 3, n)]
        s = np.select([kind == 0, kind == 1, kind == 2], [h, np.full(n, hubs[0]), h], h)
        d = np.select([kind == 0, kind == 1, kind == 2], [h, np.full(n, hubs[1]), hubs[rng.integers(0, 3, n)]],
                      cold[rng.integers(0, len(cold), n)])   # self-loops, one repeated pair, hub pairs, hub-cold
        # the second half: two ids no earlier edge names become the most frequent endpoints
        m = (np.arange(n) >= n // 2) & (rng.random(n) < 0.5)
        s[m] = late[rng.integers(0, 2, int(m.sum()))]
        lm = rng.random(int(m.sum()))
        d[m] = np.where(lm < 0.3, s[m], np.where(lm < 0.6, late[rng.integers(0, 2, int(m.sum()))], d[m]))
        _DUP["s"], _DUP["d"] = s, d
    return _DUP["s"], _DUP["d"]


@pytest.mark.parametrize("every", [2, 1000000])
@pytest.mark.parametrize("log2", [1, 3])
def test_duplicates_self_loops_and_late_ids(gs, oracle_mod, log2, every):
    s, d = _duplicates()
    _run(gs, oracle_mod, s, d, log2, every, _DUP, hint=1 << 12, check_every=1)


# ---- 5. the bucket bound ----

def test_an_index_holds_at_most_two_to_the_log2_ids(gs, oracle_mod):
    s, d, _ = _two_components()
    n = 4 * B
    ts, td = _dev(s[:n], d[:n])
    want = oracle_mod.cc_labels(s[:n], d[:n])
    held = {}
    for log2 in range(1, 21):   # every size gs_set_hot_index takes
        with gs.Summary("cc", capacity_hint=1 << 14) as ds:
            ds.set_hot_index(log2, 0, 1)
            for o in range(0, n, B):
                ds.fold_device(ts[o:], td[o:], n=B)
            held[log2] = _engaged(ds, log2)["entries"]   # asserts entries <= 1 << log2
            _equal(ds.labels(), want)
    assert held[1] <= 2
    assert held[9] > held[1]   # more buckets hold more of the hubs and their neighbours
