"""GPU: the sampling triangle estimate at the sizes its host code and kernels branch on (DESIGN.md
section 6h, "Tested").

1. the digit passes of the key sort, which the host chooses from the bits of n - 1 and S - 1:
   n and S at 256 / 257, S at 65536 / 65537, a resample key at a position >= 65536;
2. a fold with more than 1024 changed arrivals and more than 1024 rows: the carried row count of
   k_ts_rows and its read of the previous estimate across a step boundary;
3. vertices = 2^31 - 1: the third-vertex draw over the whole range, the estimate's products near
   2^31 and the saturation of Java's int cast, with changed arrivals that make no row;
4. edge counts up to 2^31 - 1 (the edge_count control): t0 + pos + 1, the coin's integer pre-test
   and the estimate at t near 2^31, the arrival limit itself, reset afterwards;
5. folds the host cuts into pieces (the piece control): summed stats, rows not kept;
6. a coin workgroup that flushes its held successes several times in one lane loop.

Truth is test_gpu_trisample.Model throughout and every comparison is exact. Each case is built by
a function that runs the model only and asserts that its input reaches the path it is named for;
those functions need no GPU."""
import functools

import numpy as np
import pytest

from test_gpu_trisample import Model, _check, _dense_stream, _rows_of, _states_of

pytestmark = pytest.mark.gpu

INT_MAX = 2147483647
ROWS_STEP = 1024  # changed arrivals per step of k_ts_rows (kTsRowsBS)
COIN_FLUSH = 192  # held successes above which a coin wave appends them (kTsCoinHold - 64)


# ---------------------------------------------------------------- one model run, any cuts
def _segments(model, src, dst, marks, snap=()):
    """Fold the model over the stream in the segments the marks cut: per segment what it adds to a
    fold (rows, coins, max_attempts) and the totals after it; the instance states only after the
    segments that end at a position of `snap` and after the last (they are large)."""
    src, dst = (np.asarray(x, dtype=np.int64) for x in (src, dst))
    bounds = [0] + sorted(set(m for m in marks if 0 < m < len(src))) + [len(src)]
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        before = model.beta_sum
        rows = model.fold(src[lo:hi].tolist(), dst[lo:hi].tolist())
        out.append({"lo": lo, "hi": hi, "rows": rows, "coins": model.coins, "max_attempts": model.max_attempts,
                    "estimate": (model.t, model.beta_sum, model.last), "changed": model.beta_sum != before,
                    "states": model.states() if hi in snap or hi == len(src) else None})
    return out


def _joined(segs, cuts=()):
    """The folds that cutting the stream at `cuts` (segment ends) makes: rows concatenated, coins
    summed, max_attempts the maximum, totals and states those after the fold's last segment."""
    assert set(cuts) <= {s["hi"] for s in segs}
    folds, cur = [], None
    for s in segs:
        if cur is None:
            cur = dict(s, rows=list(s["rows"]), pieces=1)
        else:
            cur.update(hi=s["hi"], rows=cur["rows"] + s["rows"], coins=cur["coins"] + s["coins"],
                       max_attempts=max(cur["max_attempts"], s["max_attempts"]), estimate=s["estimate"],
                       states=s["states"], pieces=cur["pieces"] + 1)
        if s["hi"] in cuts or s is segs[-1]:
            assert cur["states"] is not None
            folds.append(cur)
            cur = None
    return folds


def _same(ts, got_rows, want, pieces=1):
    """Everything _check compares, after one fold that returned got_rows; pieces > 1: the host cut
    the fold into that many device pieces, every one of which searched S carried-in segments."""
    assert got_rows == len(want["rows"])
    if pieces == 1:
        assert _rows_of(ts) == want["rows"]
    assert ts.estimate() == want["estimate"]
    assert _states_of(ts) == want["states"]
    st = ts.stats()
    assert (st["coins"], st["max_attempts"], st["rows"]) == (want["coins"], want["max_attempts"], len(want["rows"]))
    assert st["segments"] == pieces * ts.samples + want["coins"]


def _replay(gs, samples, vertices, src, dst, folds, **tune):
    """A fresh handle, tuned, folds the stream fold by fold and is compared with the model after
    each. Returns the handle's rows of all folds."""
    src, dst = (np.asarray(x, dtype=np.int64) for x in (src, dst))
    rows = []
    with gs.TriangleSampler(samples, vertices) as ts:
        ts.tune(**tune)
        for f in folds:
            _same(ts, ts.fold(src[f["lo"]:f["hi"]], dst[f["lo"]:f["hi"]]), f)
            rows += _rows_of(ts)
    return rows


# ---------------------------------------------------------------- 1. the sort's digit passes
@pytest.mark.parametrize("n", [256, 257])
@pytest.mark.parametrize("samples", [256, 257])
def test_sort_passes_at_the_first_digit_boundary_of_n_and_s(gs, samples, n):
    """Pass 1 (bits 8..15 of the position) runs iff n - 1 >= 256, pass 5 (bits 8..15 of the
    instance) iff S - 1 >= 256."""
    src, dst = _dense_stream(6, n, 300 + n)
    model, rows = _check(gs, samples, 6, src, dst, chunk=0, tile=0)
    assert rows and (model.at > 1).any()  # keys beyond arrival 1: positions differ in pass 0's digit


@pytest.mark.parametrize("samples", [65536, 65537])
def test_sort_passes_at_the_second_digit_boundary_of_s(gs, samples):
    """Pass 6 (bits 16..23 of the instance) runs iff S - 1 >= 65536. Every instance samples
    arrival 1: at least S keys, 33 tiles of the sort at 65537."""
    src, dst = _dense_stream(6, 24, 324)
    model = Model(samples, 6)
    model.fold(src[:1].tolist(), dst[:1].tolist())
    assert model.coins == samples
    _check(gs, samples, 6, src, dst, chunk=0, tile=0)


@functools.lru_cache(maxsize=None)
def _case_late_resample():
    """S = 300, 66000 arrivals over 6 vertices, recorded in the segments [0, 65536), one arrival,
    the rest. Reaches: a resample key at a position >= 65536 (bit 16 of the position: pass 2)."""
    src, dst = _dense_stream(6, 66000, 66)
    segs = _segments(Model(300, 6), src, dst, (65536, 65537), snap=(65536, 65537))
    late = [at for _, _, _, _, at in segs[-1]["states"] if at - 1 >= 65536]
    assert late, "no instance resamples at a position >= 65536"
    assert sum(s["coins"] for s in segs) > 3000 and sum(len(s["rows"]) for s in segs) > 100
    return src, dst, segs


@pytest.mark.parametrize("cuts", [(), (65536,), (65537,)])
def test_a_resample_at_a_position_past_65536(gs, cuts):
    """Whole, the fold has n - 1 >= 65536 and pass 2 runs; cut at 65536 the first fold has
    n - 1 = 65535 and skips it, cut at 65537 it has n - 1 = 65536 and runs it for one position."""
    src, dst, segs = _case_late_resample()
    rows = _replay(gs, 300, 6, src, dst, _joined(segs, cuts), chunk=0, tile=0)
    assert rows == [r for s in segs for r in s["rows"]]


# ---------------------------------------------------------------- 2. rows past one step
@functools.lru_cache(maxsize=None)
def _case_many_rows():
    """S = 1024, 1900 arrivals over 6 vertices. Reaches: more than 1024 changed arrivals and more
    than 1024 rows in one fold (counted by folding the model one arrival at a time)."""
    src, dst = _dense_stream(6, 1900, 41)
    segs = _segments(Model(1024, 6), src, dst, range(1, 1900))
    changed = sum(s["changed"] for s in segs)
    rows = [r for s in segs for r in s["rows"]]
    assert changed > ROWS_STEP and len(rows) > ROWS_STEP, (changed, len(rows))
    assert changed > len(rows)  # and some changed arrivals make no row
    return src, dst, rows


def test_more_than_one_step_of_changed_arrivals_and_rows(gs):
    import torch
    src, dst, want = _case_many_rows()
    assert _check(gs, 1024, 6, src, dst, chunk=0, tile=0)[1] == want
    assert _check(gs, 1024, 6, src, dst, cuts=[1024], chunk=0, tile=0)[1] == want
    with gs.TriangleSampler(1024, 6) as ts:
        assert ts.fold(src, dst) == len(want)
        e, est, b = (torch.full((len(want) - 1,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        with pytest.raises(gs.GSError) as err:
            ts.rows_device(e, est, b)
        assert err.value.code == gs.GS_ERR_TRUNCATED
        ts.sync()
        assert all((x == -7).all().item() for x in (e, est, b))  # untouched
        e, est, b = (torch.full((len(want),), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        assert ts.rows_device(e, est, b) == len(want)
        ts.sync()
        assert list(zip(e.tolist(), est.tolist(), b.tolist())) == want


# ---------------------------------------------------------------- 3. large vertex counts
PREFIX = 300


@functools.lru_cache(maxsize=None)
def _case_large_vertices(vertices, outside, every=256):
    """S = 4096. 300 arrivals over 12 ids drawn from [0, vertices) -- `outside`: four of them
    replaced by negative ids and ids >= vertices --, then, for every 256th (`every`) instance whose
    candidate lies inside, the two edges that close it after the prefix, (src, third) and (third, trg). Recorded arrival by
    arrival from the prefix on."""
    rng = np.random.default_rng(3)
    ids = rng.integers(0, vertices, 12)
    if outside:
        ids[[1, 4, 7, 10]] = [-1, vertices, -(1 << 40), (1 << 62) + 5]
    src, dst = ids[rng.integers(0, 12, PREFIX)], ids[rng.integers(0, 12, PREFIX)]
    model = Model(4096, vertices)
    segs = _segments(model, src, dst, ())
    assert (model.third >= 0).all() and (model.third < vertices).all()
    inside = lambda v: 0 <= v < vertices
    close_s, close_d = [], []
    for i in range(0, 4096, every):
        s, t, th = int(model.src[i]), int(model.trg[i]), int(model.third[i])
        if inside(s) and inside(t):
            close_s += [s, th]
            close_d += [th, t]
    n = PREFIX + len(close_s)
    segs += _segments(model, close_s, close_d, range(1, n))
    for s in segs[1:]:
        s["lo"], s["hi"] = s["lo"] + PREFIX, s["hi"] + PREFIX
    return np.concatenate([src, close_s]), np.concatenate([dst, close_d]), segs


def _row_facts(segs):
    """(rows below the int limit, rows at it, changed arrivals after the first such row that make
    no row) of the segments, which are single arrivals."""
    rows = [r for s in segs for r in s["rows"]]
    at_limit = [r for r in rows if r[1] == INT_MAX]
    silent = [s for s in segs
              if at_limit and s["estimate"][0] > at_limit[0][0] and s["changed"] and not s["rows"]]
    return [r for r in rows if r[1] < INT_MAX], at_limit, silent


def _replay_large_vertices(gs, vertices, src, dst, segs):
    whole = [r for s in segs for r in s["rows"]]
    assert _replay(gs, 4096, vertices, src, dst, _joined(segs), chunk=0, tile=0) == whole
    assert _replay(gs, 4096, vertices, src, dst, _joined(segs, (PREFIX,)), chunk=0, tile=0) == whole
    assert _replay(gs, 4096, vertices, src, dst, _joined(segs), chunk=8, tile=12) == whole


def test_the_largest_vertex_count_saturates_the_estimate(gs):
    """vertices = 2^31 - 1: one found triangle is worth about 1.6 * 10^8 at t = 300, the 14th
    saturates. Reaches: at least 10 rows with distinct estimates below 2^31 - 1, a row at exactly
    2^31 - 1, and after it a changed arrival that makes no row because the estimate stays there."""
    src, dst, segs = _case_large_vertices(INT_MAX, False)
    below, at_limit, silent = _row_facts(segs[1:])
    assert len({r[1] for r in below}) >= 10 and max(r[1] for r in below) > 1 << 30
    assert len(at_limit) == 1 and silent
    _replay_large_vertices(gs, INT_MAX, src, dst, segs)


def test_a_large_vertex_count_without_saturation(gs):
    vertices = 10 ** 6 + 3
    src, dst, segs = _case_large_vertices(vertices, False)
    below, at_limit, _ = _row_facts(segs[1:])
    assert len({r[1] for r in below}) >= 10 and not at_limit
    _replay_large_vertices(gs, vertices, src, dst, segs)


def test_ids_outside_a_large_vertex_range_never_close(gs):
    """Four of the 12 ids are negative or >= vertices. Reaches: candidates that contain such an id
    are held by many instances, none of them has found a side at the end, and the others close."""
    vertices = 10 ** 6 + 3
    src, dst, segs = _case_large_vertices(vertices, True, every=64)
    outside = [s for s in segs[-1]["states"] if not (0 <= s[0] < vertices and 0 <= s[1] < vertices)]
    assert len(outside) > 1000 and all(s[3] == 0 for s in outside)
    assert len(_row_facts(segs[1:])[0]) >= 5
    _replay_large_vertices(gs, vertices, src, dst, segs)


# ---------------------------------------------------------------- 4. edge counts up to 2^31 - 1
LATE_S, LATE_V, LATE_PRE, LATE_M = 4096, 10, 40, 200


@functools.lru_cache(maxsize=None)
def _case_late_edge_counts():
    """S = 4096, vertices = 10: (1.0 / 4096 * betaSum) * t * 8 passes 2^31 - 1 at t near 2^31 once
    betaSum passes 512. The prefix is 40 arrivals between distinct ids >= vertices, so that a
    candidate is shared only by the instances that sampled the same arrival and drew the same
    third vertex, about ten of them, and one pair of closing edges raises betaSum by that many. The
    model then jumps to edge count 2^31 - 1 - 200 and folds the closing edges of 100 such groups,
    recorded arrival by arrival."""
    src = 100 + 2 * np.arange(LATE_PRE, dtype=np.int64)
    dst = src + 1
    model = Model(LATE_S, LATE_V)
    pre = _segments(model, src, dst, ())
    assert model.beta_sum == 0
    groups = sorted({(int(s), int(t), int(th)) for s, t, th in zip(model.src, model.trg, model.third)})
    close_s, close_d = [], []
    for s, t, th in groups[:LATE_M // 2]:
        close_s += [s, th]
        close_d += [th, t]
    assert len(close_s) == LATE_M
    model.t = INT_MAX - LATE_M
    late = _segments(model, close_s, close_d, range(1, LATE_M), snap=(50, 51, 127))
    return (src, dst, pre[0]), (np.array(close_s), np.array(close_d), late)


def test_edge_counts_up_to_the_arrival_limit(gs):
    (psrc, pdst, pre), (src, dst, late) = _case_late_edge_counts()
    below, at_limit, silent = _row_facts(late)
    assert len(below) >= 8 and len(at_limit) == 1 and silent
    assert sum(s["coins"] for s in late) == 0  # at t near 2^31 nothing resamples
    assert max(s["estimate"][0] for s in late if s["rows"]) >= INT_MAX - LATE_M
    assert late[-1]["estimate"][0] == INT_MAX and late[-1]["estimate"][2] == INT_MAX
    whole = [r for s in late for r in s["rows"]]
    for cuts in ((), (50, 51, 127)):
        with gs.TriangleSampler(LATE_S, LATE_V) as ts:
            ts.tune(chunk=0, tile=0)
            _same(ts, ts.fold(psrc, pdst), pre)
            ts.tune(edge_count=INT_MAX - LATE_M)
            assert ts.estimate() == (INT_MAX - LATE_M,) + pre["estimate"][1:]
            assert _states_of(ts) == pre["states"] and _rows_of(ts) == pre["rows"]
            rows = []
            for f in _joined(late, cuts):
                _same(ts, ts.fold(src[f["lo"]:f["hi"]], dst[f["lo"]:f["hi"]]), f)
                rows += _rows_of(ts)
            assert rows == whole and ts.estimate()[0] == INT_MAX
            # the limit: one more arrival is refused and changes nothing
            before = (_rows_of(ts), ts.estimate(), _states_of(ts), ts.stats())
            with pytest.raises(gs.GSError) as err:
                ts.fold([1], [2])
            assert err.value.code == gs.GS_ERR_INVALID
            assert (_rows_of(ts), ts.estimate(), _states_of(ts), ts.stats()) == before
            # reset: the first-edge behaviour again, as on a fresh handle
            ts.reset()
            assert ts.estimate() == (0, 0, 0)
            _same(ts, ts.fold(psrc, pdst), pre)


# ---------------------------------------------------------------- 5. folds in pieces
@functools.lru_cache(maxsize=None)
def _case_pieces(samples, n, piece, seed):
    """n arrivals, n > piece, recorded piece by piece, then a tail of at most `piece` arrivals."""
    tail = min(piece, 40)
    src, dst = _dense_stream(6, n + tail, seed)
    segs = _segments(Model(samples, 6), src, dst, list(range(piece, n, piece)) + [n], snap=(n,))
    assert n > piece and len(segs) == -(-n // piece) + 1
    main = _joined(segs, (n,))
    assert main[0]["rows"] and main[0]["pieces"] == len(segs) - 1
    return src, dst, main


@pytest.mark.parametrize("device_arrays", [False, True])
@pytest.mark.parametrize("samples,n,piece,seed", [(65, 3 * 1024 + 5, 16, 51), (65, 3 * 1024 + 5, 1024, 51),
                                                  (300, 77, 16, 7)])
def test_a_fold_longer_than_a_piece(gs, samples, n, piece, seed, device_arrays):
    import torch
    src, dst, (main, tail) = _case_pieces(samples, n, piece, seed)
    pairs = torch.tensor(np.stack([src, dst], axis=1).reshape(-1), dtype=torch.int64, device="cuda")  # interleaved
    torch.cuda.synchronize()

    def fold(ts, lo, hi):
        if device_arrays:
            return ts.fold_device(pairs[2 * lo:], pairs[2 * lo + 1:], n=hi - lo, stride=2)
        return ts.fold(src[lo:hi], dst[lo:hi])

    with gs.TriangleSampler(samples, 6) as ts:
        ts.tune(chunk=0, tile=0, piece=piece)
        _same(ts, fold(ts, 0, n), main, pieces=main["pieces"])
        with pytest.raises(gs.GSError) as err:
            ts.rows()
        assert err.value.code == gs.GS_ERR_INVALID
        one = torch.zeros(len(main["rows"]), dtype=torch.int32, device="cuda")
        with pytest.raises(gs.GSError) as err:
            ts.rows_device(one, None, None)
        assert err.value.code == gs.GS_ERR_INVALID
        # a fold that is not longer than a piece keeps its rows again
        _same(ts, fold(ts, n, len(src)), tail)
    # the product value again: the same fold is one piece
    whole = _joined(_segments(Model(samples, 6), src[:77], dst[:77], ()))[0]
    with gs.TriangleSampler(samples, 6) as ts:
        ts.tune(piece=16)
        ts.tune(piece=0)
        _same(ts, fold(ts, 0, 77), whole)


# ---------------------------------------------------------------- 6. several flushes of a coin wave
@functools.lru_cache(maxsize=None)
def _case_coin_flushes():
    """2000 arrivals from edge count 0. Reaches: the first 64 instances -- one wave -- have more
    than 2 x 192 successes (a model of 64 samples is the first 64 instances of any larger one)."""
    src, dst = _dense_stream(6, 2000, 61)
    model = Model(64, 6)
    model.fold(src.tolist(), dst.tolist())
    assert model.coins > 2 * COIN_FLUSH, model.coins
    return src, dst


@pytest.mark.parametrize("samples", [64, 65, 300])
def test_a_coin_wave_that_flushes_several_times(gs, samples):
    """chunk = 2^30: one workgroup per 256 instances walks the whole fold, and a wave appends its
    held successes whenever they pass 192, with the count reset in between."""
    src, dst = _case_coin_flushes()
    _, rows = _check(gs, samples, 6, src, dst, chunk=1 << 30, tile=0)
    # the list overflows in the middle of a flush, is grown, and the pass runs again
    segs = _segments(Model(samples, 6), src, dst, ())
    assert _replay(gs, samples, 6, src, dst, _joined(segs), chunk=1 << 30, tile=0, keys=1) == rows
