"""GPU: the union-find fold (fold_block, combine_hooks, hook, find_root2, find_step, insert_pair)
on structured graphs cut from the kernel's own sizes -- wave 64, gsamd.FOLD_BLOCK edges per
workgroup, gsamd.FOLD_COMBINE_ROUNDS combined groups per wave -- against a sequential parity
union-find written here. Every family is one launch (or a few), so whole cycles, hubs and
duplicate runs are in flight together; every value is an integer and every comparison exact.

The rules asserted: a cycle is consistent exactly when the XOR of its edges' w is 0; a failed
verdict is sticky and its colouring empty; labels are the minimum signed id; a self-loop adds its
vertex and never fails; a tracked fold writes exactly one record per join (plus at most one per
new vertex seen through a self-loop)."""
import numpy as np
import pytest

import gsamd

pytestmark = pytest.mark.gpu

W = 64                             # lanes of a wave
BS = gsamd.FOLD_BLOCK              # edges per workgroup
ROUNDS = gsamd.FOLD_COMBINE_ROUNDS  # groups combine_hooks rewrites per wave
HINT = 1 << 13                     # no case has more than 4,096 edges: the table never grows
CAP = 1 << 13                      # record rows of a take
I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
SPECIAL = (I64_MIN, I64_MAX, -1, 0)


# ------------------------------------------------------------------ truth
def _truth(edges):
    """Sequential parity union-find over (s, d, w) triples, hooked by minimum id:
    (ok, {v: (min id of v's component, 1 when v has that vertex's colour)}, joins, index of the
    first inconsistent edge or -1). The forest goes on growing after an inconsistent edge."""
    parent, par = {}, {}

    def find(v):
        path, p = [], 0
        while parent[v] != v:
            path.append(v)
            p ^= par[v]
            v = parent[v]
        q = p
        for x in path:  # compress: q is x's parity to the root
            nxt = par[x]
            parent[x], par[x] = v, q
            q ^= nxt
        return v, p
    joins, first = 0, -1
    for i, (s, d, w) in enumerate(edges):
        for v in (s, d):
            parent.setdefault(v, v)
            par.setdefault(v, 0)
        (ra, pa), (rb, pb) = find(s), find(d)
        need = (pa ^ pb ^ w) & 1
        if ra != rb:
            parent[max(ra, rb)], par[max(ra, rb)] = min(ra, rb), need
            joins += 1
        elif need and s != d and first < 0:  # a self-loop never fails
            first = i
    col = {}
    for v in parent:
        r, p = find(v)
        col[v] = (r, 1 - p)
    return first < 0, col, joins, first


def _flat(folds):
    out = []
    for s, d, w in folds:
        out += list(zip(s, d, [1] * len(s) if w is None else w))
    return out


# ------------------------------------------------------------------ id maps
def _scramble(v):
    """Fixed and injective (an odd multiplier is a bijection of 2^64), the four special ids at
    v = 0..3."""
    if v < 4:
        return SPECIAL[v]
    z = (v * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
    return z - (1 << 64) if z >= (1 << 63) else z


assert len({_scramble(v) for v in range(1 << 13)}) == 1 << 13


def _wide_map(folds):
    """Order-preserving map of the case's ids onto wide int64 values that include the special
    ids: the family keeps its key order (a hub at the maximum stays there) at other hash slots."""
    ids = sorted({v for s, d, _ in folds for v in s + d})
    rng = np.random.default_rng(0x51DE)
    vals = set(SPECIAL[:len(ids)])
    while len(vals) < len(ids):
        vals.add(int(rng.integers(I64_MIN, I64_MAX, dtype=np.int64)))
    m = dict(zip(ids, sorted(vals)))
    return m.__getitem__


MAPS = {"identity": lambda folds: (lambda v: v), "negated": lambda folds: (lambda v: -1 - v),
        "scramble": lambda folds: _scramble, "wide": _wide_map}
MAPS3 = ("identity", "negated", "scramble")


def _mapped(folds, name):
    f = MAPS[name](folds)
    return [([f(v) for v in s], [f(v) for v in d], w) for s, d, w in folds]


# ------------------------------------------------------------------ summaries and doors
class _Pool:
    """Three summaries of each kind, shared by every case (reset_config between cases), and the
    device rows of a take."""

    def __init__(self, gs):
        import torch
        self.gs, self.torch = gs, torch
        self.sums = {k: [gs.Summary(k, capacity_hint=HINT) for _ in range(3)] for k in ("signed", "cc")}
        self.rec = torch.empty((CAP, 3), dtype=torch.int64, device="cuda")
        self.cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.exp = [torch.empty(CAP, dtype=dt, device="cuda") for dt in (torch.int64, torch.int64, torch.uint8)]
        torch.cuda.synchronize()  # filled on torch's stream; the library writes on the summary's
        self.cap0 = self.sums["cc"][0].table_capacity()

    def get(self, kind, i=0):
        x = self.sums[kind][i]
        x.reset_config()
        return x

    def dev(self, a, dtype=np.int64):
        t = self.torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()
        self.torch.cuda.synchronize()
        return t

    def close(self):
        for v in self.sums.values():
            for x in v:
                x.close()


@pytest.fixture(scope="module")
def pool(gs):
    p = _Pool(gs)
    yield p
    p.close()


def _fold_host(x, folds):
    for s, d, w in folds:
        if w is None:
            x.fold(s, d)
        else:
            x.fold_parity(s, d, w)


def _check(x, kind, T, what):
    """The summary against the truth: verdict, colouring / labels, vertex and component counts.
    (A failed fold stops wherever its workgroups first see the flag: no vertex count then.)"""
    ok, col, _, _ = T
    comps = len({c for c, _ in col.values()})
    if kind == "signed":
        gok, comp, v, sign = x.colouring()
        assert x.ok() == gok == ok, what
        if ok:
            want = sorted((c, v_, sg) for v_, (c, sg) in col.items())
            assert list(zip(comp.tolist(), v.tolist(), sign.tolist())) == want, what
            assert x.num_vertices() == len(col) and x.num_components() == comps, what
        else:
            assert len(comp) == len(v) == len(sign) == 0 and x.num_components() == 0, what
    else:
        v, lab = x.labels()
        assert list(zip(v.tolist(), lab.tolist())) == sorted((v_, c) for v_, (c, _) in col.items()), what
        assert x.num_vertices() == len(col) and x.num_components() == comps, what


def door_host(pool, kind, folds, T, what):
    """a. fold / fold_parity from host arrays."""
    x = pool.get(kind)
    _fold_host(x, folds)
    _check(x, kind, T, what)


def door_strided(pool, kind, folds, T, what):
    """b. fold_device with stride 2 (s0 d0 s1 d1 ...) and a device w."""
    x = pool.get(kind)
    keep = []
    for s, d, w in folds:
        if len(s):
            t = pool.dev(np.stack([np.asarray(s, np.int64), np.asarray(d, np.int64)], 1).ravel())
            tw = None if w is None else pool.dev(w, np.uint8)
            keep += [t, tw]
            x.fold_device(t.data_ptr(), t.data_ptr() + 8, n=len(s), stride=2, w=tw)
    _check(x, kind, T, what)


def door_pipelined(pool, kind, folds, T, what):
    """c. set_pipelining(3): every fold cut into three device folds with no sync between them."""
    x = pool.get(kind)
    x.set_pipelining(3)
    keep = []
    for s, d, w in folds:
        n = len(s)
        ts, td = pool.dev(s), pool.dev(d)
        tw = None if w is None else pool.dev(w, np.uint8)
        keep += [ts, td, tw]
        cuts = [0, n // 3, 2 * n // 3, n]
        for a, b in zip(cuts, cuts[1:]):
            if b > a:
                x.fold_device(ts.data_ptr() + 8 * a, td.data_ptr() + 8 * a, n=b - a,
                              w=None if tw is None else tw.data_ptr() + a)
    _check(x, kind, T, what)


def door_dedup(pool, kind, folds, T, what):
    """d. set_batch_dedup(True); edges without w only."""
    assert all(w is None for _, _, w in folds)
    x = pool.get(kind)
    x.set_batch_dedup(True)
    _fold_host(x, folds)
    _check(x, kind, T, what)


def _loop_vertices(fold, seen):
    return len({s for s, d in zip(fold[0], fold[1]) if s == d and s not in seen})


def _windows(folds):
    """Per fold: (truth of the stream up to and including it, joins it adds, new vertices it
    shows through a self-loop, whether the truth had failed before it)."""
    flat, seen, prev, out = [], set(), (True, {}, 0, -1), []
    for f in folds:
        flat += _flat([f])
        Tp = _truth(flat)
        out.append((Tp, Tp[2] - prev[2], _loop_vertices(f, seen), not prev[0]))
        seen |= set(f[0]) | set(f[1])
        prev = Tp
    return out


def _check_count(kind, k, word, win, gs, what):
    Tp, joins, loops, failed_before = win
    failed = kind == "signed" and not Tp[0]
    assert bool(word & gs.FAIL_BIT) == failed, what
    if kind == "signed" and failed_before:
        assert k == 0, what  # a failed verdict is final: nothing folds, nothing is recorded
    elif not failed:
        assert joins <= k <= joins + loops, (what, k, joins, loops)  # one record per successful hook CAS
    else:  # the window that fails: its workgroups stop when they see the flag, so some joins may be missing
        assert k <= joins + loops, (what, k, joins, loops)


def door_tracked(pool, kind, folds, T, what):
    """e. tracked folds, take_delta_records after each, replayed with fold_records."""
    gs = pool.gs
    x, rep = pool.get(kind), pool.get(kind, 1)
    x.set_delta_tracking(True)
    for f, win in zip(folds, _windows(folds)):
        _fold_host(x, [f])
        x.take_delta_records(pool.rec, CAP, pool.cnt)
        x.sync()
        word = int(pool.cnt.item())
        _check_count(kind, word & (gs.FAIL_BIT - 1), word, win, gs, what)
        rep.fold_records(pool.rec, word)
        rep.sync()  # rec is reused by the next take
    assert x.table_capacity() == pool.cap0, what
    _check(x, kind, T, what)
    _check(rep, kind, T, what + " (replica)")


def _door_take(pool, kind, folds, T, what, server):
    gs = pool.gs
    assert all(w is None for _, _, w in folds)
    x, rep = pool.get(kind), pool.get(kind, 1)
    x.set_delta_tracking(True)
    x.set_window_server(server)
    for (s, d, _), win in zip(folds, _windows(folds)):
        ts, td = pool.dev(s), pool.dev(d)
        k = x.fold_take(ts, td, len(s), pool.rec, CAP, pool.cnt)
        word = x.last_take_word
        assert int(pool.cnt.item()) == word, what
        _check_count(kind, k, word, win, gs, what)
        rep.fold_records(pool.rec, word)
        rep.sync()
    assert x.table_capacity() == pool.cap0, what
    _check(x, kind, T, what)
    _check(rep, kind, T, what + " (replica)")


def door_take(pool, kind, folds, T, what):
    """f. fold_take windows, a launch each."""
    _door_take(pool, kind, folds, T, what, False)


def door_take_server(pool, kind, folds, T, what):
    """f. fold_take windows through the resident window server."""
    _door_take(pool, kind, folds, T, what, True)


def _deal(folds):
    e = _flat(folds)
    halves = []
    for part in (e[0::2], e[1::2]):
        s, d, w = ([t[j] for t in part] for j in range(3))
        halves.append((s, d, w if any(f[2] is not None for f in folds) else None))
    return halves


def door_split_combine(pool, kind, folds, T, what):
    """g. the edges dealt alternately to A and B; A.combine(B)."""
    fa, fb = _deal(folds)
    a, b = pool.get(kind), pool.get(kind, 1)
    _fold_host(a, [fa])
    _fold_host(b, [fb])
    a.combine(b)
    _check(a, kind, T, what)


def door_split_exported(pool, kind, folds, T, what):
    """g. B exported with export_labels_device and folded into A with combine_exported_device."""
    fa, fb = _deal(folds)
    a, b = pool.get(kind), pool.get(kind, 1)
    _fold_host(a, [fa])
    _fold_host(b, [fb])
    v, lab, par = pool.exp
    n = b.export_labels_device(v, lab, par if kind == "signed" else None)
    failed = kind == "signed" and not b.ok()
    a.combine_exported_device(v, lab, par if kind == "signed" else None, n, failed=failed)
    _check(a, kind, T, what)


def door_split_serialized(pool, kind, folds, T, what):
    """g. B.serialize(), deserialize into a third summary, which then folds A's edges."""
    fa, fb = _deal(folds)
    b, c = pool.get(kind, 1), pool.get(kind, 2)
    _fold_host(b, [fb])
    c.deserialize(b.serialize())
    _fold_host(c, [fa])
    _check(c, kind, T, what)


BASE = (door_host, door_strided)
SPLIT = (door_split_combine, door_split_exported, door_split_serialized)
WEIGHTED = BASE + (door_pipelined, door_tracked) + SPLIT  # every door that takes a w
PLAIN = WEIGHTED + (door_dedup, door_take, door_take_server)  # and those that take none


TAIL = W + 1  # edges of the fold that follows a failing case


def _tail(folds):
    """A fold of fresh, consistent edges (a path on ids no fold has used; w alternating where the
    case has w): what a summary is given after its verdict has failed."""
    top = max(v for s, d, _ in folds for v in s + d) + 1
    weighted = any(w is not None for _, _, w in folds)
    return _fold([(top + i, top + i + 1) for i in range(TAIL)], [i & 1 for i in range(TAIL)] if weighted else None)


def _run(pool, name, folds, doors=BASE, kinds=("signed",), maps=MAPS3, expect=None):
    """One family case under each map through each door. `expect`: the verdict the family is
    built to have (checked against the truth, so a wrong generator cannot pass quietly). A case
    built to fail is followed by one more fold (_tail): the verdict is sticky, the colouring stays
    empty, and through the record doors that window has FAIL_BIT and no records."""
    if expect is False:
        folds = folds + [_tail(folds)]
    for m in maps:
        mf = _mapped(folds, m)
        T = _truth(_flat(mf))
        if expect is not None:
            assert T[0] == expect, (name, m)
        if expect is False:
            assert 0 <= T[3] < len(_flat(mf)) - TAIL, (name, m)  # the tail comes after the failure
        for kind in kinds:
            for door in doors:
                door(pool, kind, mf, T, "%s map=%s kind=%s %s" % (name, m, kind, door.__name__))


def _plain(folds):
    return [(s, d, None) for s, d, _ in folds]


def _run_plain(pool, name, folds, doors=BASE, maps=MAPS3, expect=None):
    """A family without w (every edge w = 1): kind signed and kind cc."""
    _run(pool, name, _plain(folds), doors, ("signed", "cc"), maps, expect)


def _fold(edges, w=None):
    return ([a for a, _ in edges], [b for _, b in edges], None if w is None else [int(x) for x in w])


def _strided(m):
    """Positions for m edges such that neighbours land a workgroup and a wave apart."""
    k = BS + W + 1
    while np.gcd(k, m) != 1:
        k += 1
    order = [0] * m
    for j in range(m):
        order[(j * k) % m] = j
    return order


def _positions(n):
    return sorted({p for p in (0, 1, W - 1, W, n - 1) if p < n})


# (The truth itself is compared with the oracle on the w = 1 families in tests/test_fold_capi.py,
# which needs no GPU.)


# ------------------------------------------------------------------ paths
@pytest.mark.parametrize("n", [2, W - 1, W, W + 1, BS - 1, BS, BS + 1, 4 * BS + 1])
def test_paths(pool, n):
    rng = np.random.default_rng(n)
    edges = [(i, i + 1) if i % 2 else (i + 1, i) for i in range(n - 1)]
    w = rng.integers(0, 2, n - 1)
    m = len(edges)
    orders = {"ascending": list(range(m)), "descending": list(range(m))[::-1],
              "random": rng.permutation(m).tolist(), "strided": _strided(m)}
    for oname, o in orders.items():
        f = _fold([edges[j] for j in o], w[o])
        _run(pool, "path(%d) %s" % (n, oname), [f], expect=True)
        _run_plain(pool, "path(%d) %s" % (n, oname), [f], expect=True)


# ------------------------------------------------------------------ stars
@pytest.mark.parametrize("hub", ["max", "min"])
@pytest.mark.parametrize("n", [2, W, W + 1, BS, 1000])
def test_stars(pool, n, hub):
    """Hub at the maximum key: every lane's larger root is the hub, one combine_hooks group per
    wave. Hub at the minimum: every leaf is the hooked side and becomes the hub's child, so a
    second fold of leaf-leaf edges runs the shared-parent shortcut on mixed parities."""
    rng = np.random.default_rng(n)
    h, leaves = (n, list(range(n))) if hub == "max" else (0, list(range(1, n + 1)))
    w = rng.integers(0, 2, n)
    spokes = _fold([(v, h) if i % 2 else (h, v) for i, v in enumerate(leaves)], w)
    pairs = rng.integers(0, n, (min(n, BS), 2))
    pairs[len(pairs) // 2] = (0, n - 1)  # the pair the failing case gets wrong is never a self-pair
    ww =[int(w[a] ^ w[b]) for a, b in pairs]
    second = _fold([(leaves[a], leaves[b]) for a, b in pairs], ww)
    maps = ("identity", "negated", "scramble", "wide")
    _run(pool, "star(%d) hub=%s" % (n, hub), [spokes, second], maps=maps, expect=True)
    _run_plain(pool, "star(%d) hub=%s" % (n, hub), [spokes], maps=maps, expect=True)
    p = len(ww) // 2  # (no self-pair: set above)
    ww[p] ^= 1
    bad = _fold([(leaves[a], leaves[b]) for a, b in pairs], ww)
    _run(pool, "star(%d) hub=%s, leaf pair %d wrong" % (n, hub, p), [spokes, bad], maps=maps, expect=False)


# ------------------------------------------------------------------ multi-hub waves
@pytest.mark.parametrize("k", list(range(1, ROUNDS + 3)))
def test_multi_hub_waves(pool, k):
    """k hubs at the largest keys, leaves dealt lane by lane: every wave holds k groups, of which
    combine_hooks rewrites ROUNDS; the others contend on their hub's link in the hook loop."""
    rng = np.random.default_rng(k)
    edges = [(i, BS + i % k) for i in range(BS)]
    w = rng.integers(0, 2, BS)
    maps = ("identity", "wide", "negated", "scramble")
    _run(pool, "%d hubs" % k, [_fold(edges, w)], WEIGHTED, maps=maps, expect=True)
    _run_plain(pool, "%d hubs" % k, [_fold(edges)], PLAIN, maps=maps, expect=True)
    # two leaves under two hubs each close the cycle 0 - h0 - 1 - h1 - 0 among the groups: the
    # XOR of its four w is `bad`
    for bad in (0, 1) if k >= 2 else ():
        tie = _fold(edges + [(0, BS + 1), (1, BS)], list(w) + [int(w[0]), int(w[1]) ^ bad])
        _run(pool, "%d hubs tied xor=%d" % (k, bad), [tie], WEIGHTED, maps=("identity", "wide"), expect=bad == 0)


# ------------------------------------------------------------------ duplicates
@pytest.mark.parametrize("n", [W, BS, 1000])
def test_duplicates(pool, n):
    e = [(3, 7) if i % 3 else (7, 3) for i in range(n)]
    for w0 in (0, 1):
        _run(pool, "%d duplicates w=%d" % (n, w0), [_fold(e, [w0] * n)], WEIGHTED, expect=True)
        for p in _positions(n):
            w = [w0] * n
            w[p] ^= 1
            _run(pool, "%d duplicates, w differs at %d" % (n, p), [_fold(e, w)], WEIGHTED, expect=False)
    _run_plain(pool, "%d duplicates" % n, [_fold(e)], PLAIN, expect=True)
    # id -1 is the dedup table's empty marker: such an edge is never dropped, and still folds
    raw = [(-1, 5) if i % 2 else (5, -1) for i in range(n)] + [(-1, -1), (9, -1)]
    _run_plain(pool, "%d duplicates of (-1, 5)" % n, [_fold(raw)], (door_dedup, door_take, door_host),
               maps=("identity",), expect=True)


# ------------------------------------------------------------------ cycles
def _rotations(edges, w):
    """The closing (last-indexed) edge first, in the middle and last."""
    m = len(edges)
    for name, at in (("first", 0), ("middle", (m - 1) // 2), ("last", m - 1)):
        o = list(range(m - 1))
        o.insert(at, m - 1)
        yield name, [edges[j] for j in o], [int(w[j]) for j in o]


@pytest.mark.parametrize("k", [3, 4, 5, 6, W - 1, W, W + 1, BS - 1, BS, BS + 1])
def test_cycles(pool, k):
    """C_k with every edge in one fold call: consistent exactly when the XOR of its w is 0."""
    rng = np.random.default_rng(k)
    edges = [(i, (i + 1) % k) for i in range(k)]
    for x in (0, 1):
        w = rng.integers(0, 2, k)
        w[int(rng.integers(k))] ^= (int(w.sum()) & 1) ^ x  # force the XOR to x
        assert int(np.bitwise_xor.reduce(w)) == x
        for rname, e, ww in _rotations(edges, w):
            _run(pool, "C_%d xor=%d closing edge %s" % (k, x, rname), [_fold(e, ww)], WEIGHTED, expect=x == 0)
    for rname, e, _ in _rotations(edges, [1] * k):
        _run_plain(pool, "C_%d closing edge %s" % (k, rname), [_fold(e)], PLAIN, expect=k % 2 == 0)
    if k % 2 == 0:  # alternating colours
        _, col, _, _ = _truth(_flat([_fold(edges)]))
        assert all(col[v] == (0, 1 - v % 2) for v in range(k))


@pytest.mark.parametrize("shape", ["triangles", "squares"])
def test_many_cycles_at_once(pool, shape):
    """Disjoint small cycles closing together in one workgroup: no false failure among them,
    and one inconsistent cycle among them is found."""
    k, count, w = (3, (BS - 1) // 3, [1, 1, 0]) if shape == "triangles" else (4, BS // 4, [1, 1, 1, 1])
    assert count in (85, 64)
    cyc = [[(k * t + i, k * t + (i + 1) % k) for i in range(k)] for t in range(count)]
    layouts = {"cycle by cycle": [(t, i) for t in range(count) for i in range(k)],
               "edge by edge": [(t, i) for i in range(k) for t in range(count)]}
    for lname, lay in layouts.items():
        e = [cyc[t][i] for t, i in lay]
        _run(pool, "%d %s %s" % (count, shape, lname), [_fold(e, [w[i] for _, i in lay])], WEIGHTED, expect=True)
        if shape == "squares":
            _run_plain(pool, "%d squares %s" % (count, lname), [_fold(e)], PLAIN, expect=True)
        for bad in (0, count // 2, count - 1):
            ww = [w[i] ^ (1 if (t, i) == (bad, k - 1) else 0) for t, i in lay]
            _run(pool, "%d %s %s, cycle %d odd" % (count, shape, lname, bad), [_fold(e, ww)], WEIGHTED,
                 maps=("identity", "scramble"), expect=False)
    if shape == "triangles":  # unweighted they are all odd, through the doors that take no w
        _run_plain(pool, "%d odd triangles" % count, [_fold([cyc[t][i] for t, i in layouts["cycle by cycle"]])],
                   (door_host, door_dedup, door_take, door_take_server), expect=False)


# ------------------------------------------------------------------ complete bipartite graphs
@pytest.mark.parametrize("a,b", [(2, 64), (8, 32)])
def test_complete_bipartite(pool, a, b):
    edges = [(i, a + j) for j in range(b) for i in range(a)]
    ones = [1] * len(edges)
    _run_plain(pool, "K_%d,%d" % (a, b), [_fold(edges)], expect=True)
    same = [(0, 1), (a, a + 1), (a + 2, a + b - 1)]  # same-side pairs: left, right, right
    for u, v in same:
        for w in (1, 0):
            _run(pool, "K_%d,%d + (%d,%d) w=%d" % (a, b, u, v, w), [_fold(edges + [(u, v)], ones + [w])],
                 expect=w == 0)
            _run(pool, "K_%d,%d, then (%d,%d) w=%d" % (a, b, u, v, w), [_fold(edges, ones), _fold([(u, v)], [w])],
                 expect=w == 0)
    # every same-side pair of the right side at once, after the graph: siblings and parent/child
    pairs = [(a + i, a + j) for i in range(b) for j in range(i + 1, b)][:4 * BS]
    _run(pool, "K_%d,%d, then same-side pairs w=0" % (a, b), [_fold(edges, ones), _fold(pairs, [0] * len(pairs))],
         expect=True)
    _run_plain(pool, "K_%d,%d + (0,1)" % (a, b), [_fold(edges + [(0, 1)])], expect=False)


# ------------------------------------------------------------------ two trees, many bridges
@pytest.mark.parametrize("m", [1, W, BS])
@pytest.mark.parametrize("trees", ["paths", "stars"])
def test_two_trees_many_bridges(pool, trees, m):
    """Fold 1 builds two trees; fold 2 is m parallel edges between them: one hook wins, the
    others meet a == b in the retry loop and must agree with the two colourings."""
    rng = np.random.default_rng(m)
    P = W
    if trees == "paths":
        t1 = [(i, i + 1) for i in range(P - 1)] + [(P + i, P + i + 1) for i in range(P - 1)]
    else:
        t1 = [(0, i) for i in range(1, P)] + [(2 * P - 1, P + i) for i in range(P - 1)]
    w1 = rng.integers(0, 2, len(t1))
    _, col, _, _ = _truth(_flat([_fold(t1, w1)]))
    assert len({c for c, _ in col.values()}) == 2
    delta = int(rng.integers(2))
    ends = [(int(rng.integers(P)), P + int(rng.integers(P))) for _ in range(m)]
    ends = [(u, v) if i % 2 else (v, u) for i, (u, v) in enumerate(ends)]
    w2 = [col[u][1] ^ col[v][1] ^ delta for u, v in ends]
    _run(pool, "%s, %d bridges" % (trees, m), [_fold(t1, w1), _fold(ends, w2)], WEIGHTED, expect=True)
    for p in _positions(m) if m > 1 else ():
        ww = list(w2)
        ww[p] ^= 1
        _run(pool, "%s, %d bridges, wrong at %d" % (trees, m, p), [_fold(t1, w1), _fold(ends, ww)], WEIGHTED,
             expect=False)
    # unweighted: the trees are bipartite, a bridge set is consistent when every bridge joins
    # the same pair of colour classes
    plain1 = _truth(_flat([_fold(t1)]))[1]
    a0 = [v for v in range(P) if plain1[v][1]]
    b0 = [v for v in range(P, 2 * P) if plain1[v][1]]
    br = [(a0[int(rng.integers(len(a0)))], b0[int(rng.integers(len(b0)))]) for _ in range(m)]
    _run_plain(pool, "%s, %d bridges" % (trees, m), [_fold(t1), _fold(br)], PLAIN, expect=True)
    if m > 1:
        other = [v for v in range(P, 2 * P) if not plain1[v][1]][0]
        for p in _positions(m):
            bad = list(br)
            bad[p] = (bad[p][0], other)
            _run_plain(pool, "%s, %d bridges, odd at %d" % (trees, m, p), [_fold(t1), _fold(bad)], PLAIN,
                       maps=("identity", "scramble"), expect=False)


# ------------------------------------------------------------------ deep chain
@pytest.mark.parametrize("mapname", ["identity", "negated", "wide"])
@pytest.mark.parametrize("last", ["host", "strided"])
@pytest.mark.parametrize("bad", [False, True])
def test_deep_chain(pool, mapname, bad, last):
    """2 * BS single-edge device folds, each hooking the previous root under a smaller key: a
    chain 2 * BS links deep with mixed parities. One fold of BS edges (from host arrays, or
    strided device arrays) then walks it from the deep end and from random vertices, path
    splitting on the way, while other lanes read the same links. (The maps are the monotone ones:
    under the scramble the keys are in no order and the tree stays shallow.)"""
    import torch
    N = 2 * BS
    rng = np.random.default_rng(7)
    w = rng.integers(0, 2, N)
    colour = np.concatenate([[0], np.bitwise_xor.accumulate(w)])  # of vertex i, against vertex 0
    up = mapname == "negated"  # the smaller key of (i, i + 1) must arrive last
    chain = [((i, i + 1), int(w[i])) for i in (range(N) if up else range(N - 1, -1, -1))]
    deep = 0 if up else N
    fresh = iter(range(N + 1, 2 * N))
    e2, w2 = [], []
    for j in range(BS):
        u = deep if j % 4 == 0 else int(rng.integers(N + 1))
        if j % 2:
            v = int(rng.integers(N + 1))
            e2.append((u, v))
            w2.append(int(colour[u] ^ colour[v]))
        else:
            e2.append((u, next(fresh)) if j % 3 else (next(fresh), u))
            w2.append(int(rng.integers(2)))
    if bad:
        p = next(j for j in range(BS // 2, BS) if j % 2 and e2[j][0] != e2[j][1])
        w2[p] ^= 1
    o = rng.permutation(BS)
    folds = [_fold([e], [x]) for e, x in chain] + [_fold([e2[j] for j in o], [w2[j] for j in o])]
    mf = _mapped(folds, mapname)
    T = _truth(_flat(mf))
    assert T[0] == (not bad)
    x = pool.get("signed")
    flat = _flat(mf)
    ts, td = pool.dev([e[0] for e in flat]), pool.dev([e[1] for e in flat])
    tw = pool.dev([e[2] for e in flat], np.uint8)
    for i in range(N):
        x.fold_device(ts.data_ptr() + 8 * i, td.data_ptr() + 8 * i, n=1, w=tw.data_ptr() + i)
    s2, d2, w2 = mf[-1]
    if last == "host":
        x.fold_parity(s2, d2, w2)
    else:
        t2 = pool.dev(np.stack([np.asarray(s2, np.int64), np.asarray(d2, np.int64)], 1).ravel())
        x.fold_device(t2.data_ptr(), t2.data_ptr() + 8, n=BS, stride=2, w=tw.data_ptr() + N)
    what = "deep chain map=%s bad=%s last=%s" % (mapname, bad, last)
    _check(x, "signed", T, what)
    if not bad:
        col = T[1]
        v, lab = x.labels()
        assert list(zip(v.tolist(), lab.tolist())) == sorted((v_, c) for v_, (c, _) in col.items()), what
        q = sorted(col) + [123456789]
        tq = pool.dev(q)
        out = torch.empty_like(tq)
        found = torch.empty(len(q), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        x.find_labels_device(tq, out, found)
        x.sync()
        assert out.cpu().tolist()[:-1] == [col[v_][0] for v_ in q[:-1]], what
        assert found.cpu().tolist() == [1] * (len(q) - 1) + [0], what


# ------------------------------------------------------------------ self-loops
def test_self_loops(pool):
    """A self-loop adds its vertex and never fails, whatever its w; its only record is the one
    that names a new vertex."""
    rng = np.random.default_rng(3)
    n = BS + 1
    loops = [(v, v) for v in range(n)]
    for w0 in (0, 1):
        _run(pool, "%d self-loops w=%d" % (n, w0), [_fold(loops, [w0] * n)], WEIGHTED, expect=True)
    _run_plain(pool, "%d self-loops" % n, [_fold(loops), _fold(loops[::2])], PLAIN, expect=True)
    # mixed into a star: loops on the hub, on leaves and on vertices seen nowhere else
    star = [(v, n) for v in range(n)]
    extra = [(n, n), (0, 0), (W, W), (n + 1, n + 1), (n + 2, n + 2)] * 3
    e = star + extra
    w = rng.integers(0, 2, len(e))
    o = rng.permutation(len(e))
    f = _fold([e[j] for j in o], w[o])
    _run(pool, "star with self-loops", [f], WEIGHTED, maps=("identity", "negated", "scramble", "wide"), expect=True)
    _run_plain(pool, "star with self-loops", [f], PLAIN, expect=True)


# ------------------------------------------------------------------ the delta list's shards
@pytest.mark.parametrize("kind", ["signed", "cc"])
def test_tracked_folds_wrap_the_shards(pool, kind):
    """gsamd.FOLD_SHARDS + 1 tracked one-workgroup folds before a single take: every launch
    starts one shard after the previous one, so the records lie in every shard of the delta list
    and the last fold comes round to the first shard again. The take gathers them all: exactly
    one record per join, and their replay rebuilds the summary."""
    gs = pool.gs
    rng = np.random.default_rng(11)
    folds = []
    for f in range(gsamd.FOLD_SHARDS + 1):  # a comb: the spine grows by one vertex and one tooth per fold
        w = [int(x) for x in rng.integers(0, 2, 2)]
        folds.append(_fold([(f, f + 1), (1000 + f, f), (f + 1, f)], w + [w[0]]))
    if kind == "cc":
        folds = _plain(folds)
    for m in MAPS3:
        mf = _mapped(folds, m)
        T = _truth(_flat(mf))
        assert T[0] and T[2] == 2 * len(folds)
        x, rep = pool.get(kind), pool.get(kind, 1)
        x.set_delta_tracking(True)
        _fold_host(x, mf)
        x.take_delta_records(pool.rec, CAP, pool.cnt)
        x.sync()
        word = int(pool.cnt.item())
        what = "comb over %d folds map=%s kind=%s" % (len(folds), m, kind)
        assert word == T[2], what
        rep.fold_records(pool.rec, word)
        rep.sync()
        assert x.table_capacity() == pool.cap0, what
        _check(x, kind, T, what)
        _check(rep, kind, T, what + " (replica)")
