"""GPU: the sampling triangle estimate (gs_trisample_*, gsamd.TriangleSampler) against a model
written from the contract in include/gs_summary.h (java.util.Random's LCG, the coin, the
counter-based third vertex, the candidate state machine, the row rule, Java's int cast): the rows,
betaSum, the estimate and every instance's state must equal the model exactly, wherever the stream
is cut into folds and wherever the coin pass's chunks and the search pass's tiles end. The model
is vectorised over the instances and loops over the arrivals; every case keeps
instances x arrivals below 2 * 10^6. Beside it the pins of tests/golden/trisample_pins.json and a
statistical sanity check of the estimate against the exact count of gsamd.Triangles."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M48, M64, MULT = (1 << 48) - 1, (1 << 64) - 1, 0x5DEECE66D
CHUNK, TILE = 8, 12  # the testing overrides of most cases: boundaries every few arrivals


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _signed32(x):
    return x - (1 << 32) if x >> 31 else x


def _instance_seeds(master, count):
    """(long) master.nextInt(), count times, of new Random(master)."""
    s, out = (master ^ MULT) & M48, []
    for _ in range(count):
        s = (s * MULT + 0xB) & M48
        out.append(_signed32(s >> 16))
    return out


def _java_int(x):
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def _third(third_seed, instance, t, vertices, src, trg):
    h = _mix64((third_seed + 0x9E3779B97F4A7C15 * (instance + 1)) & M64)
    h = _mix64(h ^ t)
    a = 0
    while True:
        x = _mix64(h ^ a)
        third = int(math.floor(float(x >> 11) * 2.0 ** -53 * float(vertices)))
        a += 1
        if third != src and third != trg:
            return third, a


class Model:
    def __init__(self, samples, vertices, seed=-559038737, third_seed=0):
        self.S, self.V, self.third_seed = samples, vertices, third_seed
        self.lcg = np.array([(x ^ MULT) & M48 for x in _instance_seeds(seed, samples)], dtype=np.uint64)
        self.src = np.zeros(samples, np.int64)
        self.trg = np.zeros(samples, np.int64)
        self.third = np.full(samples, -1, np.int64)
        self.sf, self.tf, self.beta = (np.zeros(samples, bool) for _ in range(3))
        self.at = np.zeros(samples, np.int32)
        self.t = self.beta_sum = self.last = self.coins = self.max_attempts = 0

    def fold(self, src, dst):
        """The rows (edges, estimate, betaSum) of one fold."""
        rows = []
        self.coins = self.max_attempts = 0
        mult, add, mask = np.uint64(MULT), np.uint64(0xB), np.uint64(M48)
        for a, b in zip(src, dst):
            a, b = int(a), int(b)
            self.t += 1
            t = self.t
            s1 = (self.lcg * mult + add) & mask
            s2 = (s1 * mult + add) & mask
            self.lcg = s2
            nd = (((s1 >> np.uint64(22)) << np.uint64(27)) + (s2 >> np.uint64(21))).astype(np.float64) * 2.0 ** -53
            for i in np.nonzero(nd * float(t) <= 1.0)[0].tolist():
                third, attempts = _third(self.third_seed, i, t, self.V, a, b)
                self.src[i], self.trg[i], self.third[i] = a, b, third
                self.sf[i] = self.tf[i] = self.beta[i] = False
                self.at[i] = t
                self.coins += 1
                self.max_attempts = max(self.max_attempts, attempts)
            open_ = ~self.beta
            self.sf |= open_ & (((self.src == a) & (self.third == b)) | ((self.third == a) & (self.src == b)))
            self.tf |= open_ & (((self.trg == a) & (self.third == b)) | ((self.third == a) & (self.trg == b)))
            self.beta = self.sf & self.tf
            bs = int(self.beta.sum())
            if bs != self.beta_sum:
                self.beta_sum = bs
                est = _java_int((((1.0 / self.S) * bs) * t) * (self.V - 2))
                if est != self.last:
                    self.last = est
                    rows.append((t, est, bs))
        return rows

    def states(self):
        flags = self.sf.astype(int) + 2 * self.tf.astype(int) + 4 * self.beta.astype(int)
        return list(zip(self.src.tolist(), self.trg.tolist(), self.third.tolist(), flags.tolist(), self.at.tolist()))


def _rows_of(ts):
    e, est, b = ts.rows()
    return list(zip(e.tolist(), est.tolist(), b.tolist()))


def _states_of(ts):
    return list(zip(*(x.tolist() for x in ts.states())))


def _check(gs, samples, vertices, src, dst, cuts=(), chunk=CHUNK, tile=TILE, seed=-559038737, third_seed=0):
    """Fold the stream (whole, or cut at `cuts`) and compare everything with the model after every
    fold; returns the model and the rows of all folds."""
    src, dst = (np.asarray(x, dtype=np.int64) for x in (src, dst))
    bounds = [0] + sorted(set(c for c in cuts if 0 < c < len(src))) + [len(src)]
    model = Model(samples, vertices, seed, third_seed)
    rows = []
    with gs.TriangleSampler(samples, vertices, seed=seed, third_seed=third_seed) as ts:
        ts.tune(chunk=chunk, tile=tile)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            want = model.fold(src[lo:hi].tolist(), dst[lo:hi].tolist())
            assert ts.fold(src[lo:hi], dst[lo:hi]) == len(want)
            assert _rows_of(ts) == want
            assert ts.estimate() == (model.t, model.beta_sum, model.last)
            assert _states_of(ts) == model.states()
            st = ts.stats()
            assert (st["coins"], st["max_attempts"], st["rows"]) == (model.coins, model.max_attempts, len(want))
            assert st["segments"] == samples + model.coins
            rows += want
    return model, rows


def _dense_stream(vertices, n, seed):
    """n arrivals over few vertices, repeats, both directions and self-loops included."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, vertices, n), rng.integers(0, vertices, n)


def _complete(v):
    return [a for a in range(v) for b in range(a + 1, v)], [b for a in range(v) for b in range(a + 1, v)]


@functools.lru_cache(maxsize=None)
def _random_graph(vertices=24, density=0.6, seed=5):
    """A simple graph, every edge once, in random order."""
    rng = np.random.default_rng(seed)
    pairs = [(a, b) for a in range(vertices) for b in range(a + 1, vertices) if rng.random() < density]
    order = rng.permutation(len(pairs))
    flip = rng.random(len(pairs)) < 0.5
    src = [pairs[k][1] if flip[k] else pairs[k][0] for k in order]
    dst = [pairs[k][0] if flip[k] else pairs[k][1] for k in order]
    return tuple(src), tuple(dst)


# n around the chunk (8) and tile (12) overrides: size - 1, size, size + 1 and 3 x size + 5
SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, TILE - 1, TILE, TILE + 1, 3 * CHUNK + 5, 3 * TILE + 5)


@pytest.mark.parametrize("samples", [1, 63, 64, 65, 300])
def test_every_size_around_chunk_and_tile(gs, samples):
    for n in SIZES:
        src, dst = _dense_stream(6, n, 100 + n)
        _, rows = _check(gs, samples, 6, src, dst)
        if samples >= 63 and n >= 3 * CHUNK:
            assert rows  # the streams do make rows


@pytest.mark.parametrize("samples", [1, 63, 64, 65, 300])
def test_folds_cut_at_every_boundary_and_into_single_arrivals(gs, samples):
    n = 3 * TILE + 5
    src, dst = _dense_stream(6, n, 7)
    whole = _check(gs, samples, 6, src, dst)[1]
    assert _check(gs, samples, 6, src, dst, cuts=SIZES)[1] == whole
    assert _check(gs, samples, 6, src, dst, cuts=range(1, n))[1] == whole
    # a second fold after t0 > 0, at the product's chunk and tile
    assert _check(gs, samples, 6, src, dst, cuts=[17], chunk=0, tile=0)[1] == whole


def test_product_chunk_and_tile_boundaries(gs):
    n = gs.TRISAMPLE_TILE + gs.TRISAMPLE_CHUNK + 7
    src, dst = _dense_stream(9, n, 11)
    whole = _check(gs, 65, 9, src, dst, chunk=0, tile=0)[1]
    assert whole
    cuts = [gs.TRISAMPLE_CHUNK - 1, gs.TRISAMPLE_CHUNK, gs.TRISAMPLE_TILE, gs.TRISAMPLE_TILE + 1]
    assert _check(gs, 65, 9, src, dst, cuts=cuts, chunk=0, tile=0)[1] == whole
    assert _check(gs, 65, 9, src, dst, chunk=1, tile=1)[1] == whole


def test_a_resample_list_too_small_is_grown_and_the_coin_pass_run_again(gs):
    src, dst = _dense_stream(6, 3 * TILE + 5, 7)
    model = Model(300, 6)
    with gs.TriangleSampler(300, 6) as ts:
        ts.tune(chunk=CHUNK, tile=TILE, keys=1)  # (every instance samples the first edge: 300 keys at least)
        for lo, hi in ((0, 20), (20, 41)):
            want = model.fold(src[lo:hi].tolist(), dst[lo:hi].tolist())
            assert ts.fold(src[lo:hi], dst[lo:hi]) == len(want) and _rows_of(ts) == want
            assert ts.stats()["coins"] == model.coins >= 1 and _states_of(ts) == model.states()
        assert ts.estimate() == (model.t, model.beta_sum, model.last)


def test_pinned_k5_stream(gs):
    with open(os.path.join(ROOT, "tests", "golden", "trisample_pins.json")) as f:
        pin = json.load(f)["k5_twice"]
    src, dst = _complete(5)
    model, rows = _check(gs, pin["samples"], pin["vertices"], src * 2, dst * 2, third_seed=pin["third_seed"])
    assert [list(r[:2]) for r in rows] == pin["rows"]
    assert model.beta_sum == pin["beta_sum"]
    assert [[s, t, th, bool(f & 1), bool(f & 2), f >> 2, at] for s, t, th, f, at in model.states()] == pin["states"]
    assert rows[2][1] < rows[1][1]  # the row at 15 is a decrease: a resample kills a found triangle
    for cuts in ([7, 8], [14, 15], range(1, 20)):
        assert _check(gs, 4, 5, src * 2, dst * 2, cuts=cuts)[1] == rows


def test_k16_makes_a_hundred_rows(gs):
    src, dst = _complete(16)
    _, rows = _check(gs, 2048, 16, src, dst, chunk=0, tile=0)
    assert len(rows) == 100
    assert _check(gs, 2048, 16, src, dst, cuts=[1, 50, 51, 119])[1] == rows


def test_random_graph(gs):
    src, dst = _random_graph()
    _, rows = _check(gs, 300, 24, src, dst)
    assert len(rows) > 10
    assert _check(gs, 300, 24, src, dst, cuts=[1, 2, 64, 100], chunk=0, tile=0)[1] == rows


def test_corner_streams(gs):
    # duplicate arrivals and reversed directions
    src, dst = _complete(6)
    _check(gs, 65, 6, src + dst + src, dst + src + src)
    # a self-loop sampled at t = 1, then one edge to its third vertex: that edge sets both flags
    third, _ = _third(3, 0, 1, 5, 2, 2)
    model, _ = _check(gs, 1, 5, [2, third], [2, 2], third_seed=3)
    if model.at[0] == 1:  # (not resampled at t = 2)
        assert model.states()[0] == (2, 2, third, 7, 1)
    seen = 0
    for third_seed in range(8):  # some of these keep the first candidate
        third, _ = _third(third_seed, 0, 1, 5, 2, 2)
        model, rows = _check(gs, 1, 5, [2, 2], [2, third], third_seed=third_seed)
        seen += model.states()[0][3] == 7
    assert seen >= 1
    # ids outside [0, vertices), negative ones included: they are sampled, and never closed
    big = (1 << 62) + 5
    src = [big, -3, big, 1, -3, 2, big, -3, 1, 0]
    dst = [-3, big, 1, big, 2, -3, -3, big, 2, 1]
    model, _ = _check(gs, 300, 4, src * 3, dst * 3)
    assert any(s[0] == big or s[1] == -3 for s in model.states())
    # the smallest vertex count: the third vertex is the one left
    src, dst = _dense_stream(3, 40, 3)
    model, rows = _check(gs, 65, 3, src, dst)
    assert rows and model.max_attempts > 1


def test_reset_restores_the_first_edge_behaviour(gs):
    src, dst = _dense_stream(6, 30, 21)
    with gs.TriangleSampler(65, 6) as ts:
        ts.tune(chunk=CHUNK, tile=TILE)
        assert _states_of(ts) == [(0, 0, -1, 0, 0)] * 65
        assert ts.estimate() == (0, 0, 0)
        ts.fold(src, dst)
        first = (_rows_of(ts), ts.estimate(), _states_of(ts))
        assert all(s[4] >= 1 for s in first[2])
        ts.reset()
        assert ts.estimate() == (0, 0, 0) and _states_of(ts) == [(0, 0, -1, 0, 0)] * 65
        assert ts.stats() == {"coins": 0, "segments": 0, "max_attempts": 0, "rows": 0}
        ts.fold(src, dst)
        assert (_rows_of(ts), ts.estimate(), _states_of(ts)) == first
        assert ts.stats()["coins"] >= 65  # every instance samples the first edge again


def test_device_pointer_variants_with_stride(gs):
    import torch
    src, dst = _random_graph()
    n = len(src)
    model = Model(300, 24)
    want = model.fold(src[:100], dst[:100])
    want2 = model.fold(src[100:], dst[100:])
    pairs = torch.tensor(np.stack([src, dst], axis=1).reshape(-1), dtype=torch.int64, device="cuda")  # interleaved
    torch.cuda.synchronize()
    with gs.TriangleSampler(300, 24) as ts:
        assert ts.fold_device(pairs, pairs[1:], n=100, stride=2) == len(want)
        e, est, b = (torch.zeros(max(len(want), 1), dtype=torch.int32, device="cuda") for _ in range(3))
        ts.wait_stream()
        assert ts.rows_device(e, est, b) == len(want)
        ts.sync()
        assert list(zip(e.tolist(), est.tolist(), b.tolist()))[:len(want)] == want
        assert ts.fold_device(pairs[200:], pairs[201:], n=n - 100, stride=2) == len(want2)
        assert _rows_of(ts) == want2
        small = torch.zeros(1, dtype=torch.int32, device="cuda")
        if len(want2) > 1:
            with pytest.raises(gs.GSError) as err:
                ts.rows_device(small, None, None)
            assert err.value.code == gs.GS_ERR_TRUNCATED
        s, t, th = (torch.zeros(300, dtype=torch.int64, device="cuda") for _ in range(3))
        f = torch.zeros(300, dtype=torch.uint8, device="cuda")
        at = torch.zeros(300, dtype=torch.int32, device="cuda")
        ts.wait_stream()
        ts.states_device(s, t, th, f, at)
        ts.sync()
        assert list(zip(s.tolist(), t.tolist(), th.tolist(), f.tolist(), at.tolist())) == model.states()
        assert ts.estimate() == (model.t, model.beta_sum, model.last)


def test_total_arrivals_are_limited_and_the_state_is_untouched(gs):
    import torch
    src, dst = _dense_stream(6, 20, 2)
    L = gs.lib()
    with gs.TriangleSampler(64, 6) as ts:
        ts.fold(src, dst)
        before = (_rows_of(ts), ts.estimate(), _states_of(ts), ts.stats())
        d = torch.zeros(8, dtype=torch.int64, device="cuda")
        rows = ctypes.c_size_t(77)
        too_many = gs.TRISAMPLE_MAX_ARRIVALS - 20 + 1
        assert L.gs_trisample_fold_device(ts.handle, d.data_ptr(), d.data_ptr(), too_many, 1,
                                          ctypes.byref(rows)) == gs.GS_ERR_INVALID
        assert b"2^31 - 1" in L.gs_last_error() and rows.value == 77
        assert L.gs_trisample_fold_device(ts.handle, d.data_ptr(), d.data_ptr(), 4, 0, None) == gs.GS_ERR_INVALID
        assert L.gs_trisample_fold(ts.handle, None, None, 3, None) == gs.GS_ERR_INVALID
        assert (_rows_of(ts), ts.estimate(), _states_of(ts), ts.stats()) == before
        assert ts.fold([], []) == 0 and ts.estimate() == before[1]


def test_estimate_is_within_five_sigma_of_the_exact_count(gs):
    """On a simple graph with no repeated edge a candidate closes with probability
    p = T / (E (V - 2)) -- a triangle counts only when its first-arriving edge is the sample -- so
    betaSum / S * E * (V - 2) estimates T with sigma = E (V - 2) sqrt(p (1 - p) / S). Five sigma: the
    run is deterministic and must not sit on an edge (for this graph the model gives 517.8 against
    T = 515 with sigma = 20.4)."""
    src, dst = _random_graph()
    S, V, E = 4096, 24, len(src)
    with gs.Triangles() as tri:
        tri.fold(src, dst)
        T, edges, _ = tri.count()
    assert edges == E and T > 100
    model = Model(S, V)
    model.fold(src, dst)
    with gs.TriangleSampler(S, V) as ts:
        ts.fold(src, dst)
        arrivals, beta_sum, _ = ts.estimate()
    assert (arrivals, beta_sum) == (E, model.beta_sum)
    p = T / (E * (V - 2))
    sigma = E * (V - 2) * math.sqrt(p * (1 - p) / S)
    estimate = beta_sum / S * E * (V - 2)
    print("T = %d, E = %d, estimate = %.1f, sigma = %.1f" % (T, E, estimate, sigma))
    assert abs(estimate - T) <= 5 * sigma
