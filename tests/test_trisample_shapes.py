"""CPU: the inputs of test_gpu_trisample_shapes.py reach the paths those tests are named for. The
case builders run the model only and assert their own conditions; here they are run without a
GPU, with the figures the model gives for them. Pure Python: no library is loaded."""
import test_gpu_trisample_shapes as shapes
from test_gpu_trisample import Model, _dense_stream

INT_MAX = shapes.INT_MAX


def test_a_fold_has_a_resample_key_at_a_position_past_65536():
    src, dst, segs = shapes._case_late_resample()
    assert len(src) == 66000 and [s["hi"] for s in segs] == [65536, 65537, 66000]
    at = {i: s[4] for i, s in enumerate(segs[-1]["states"]) if s[4] > 65536}
    assert at == {153: 65977, 241: 65834}  # positions 65976 and 65833
    assert sum(s["coins"] for s in segs) == 3577
    whole = shapes._joined(segs)
    assert len(whole) == 1 and whole[0]["coins"] == 3577 and whole[0]["pieces"] == 3
    assert [f["hi"] for f in shapes._joined(segs, (65536,))] == [65536, 66000]


def test_a_fold_has_more_than_a_step_of_changed_arrivals_and_of_rows():
    src, dst, rows = shapes._case_many_rows()
    model = Model(1024, 6)
    changed = 0
    for a, b in zip(src.tolist(), dst.tolist()):
        before = model.beta_sum
        model.fold([a], [b])
        changed += model.beta_sum != before
    assert (changed, len(rows)) == (1392, 1229) and shapes.ROWS_STEP == 1024


def test_large_vertex_counts_saturate_or_do_not():
    src, dst, segs = shapes._case_large_vertices(INT_MAX, False)
    below, at_limit, silent = shapes._row_facts(segs[1:])
    assert len(src) == 332 and segs[0]["hi"] == shapes.PREFIX and segs[0]["estimate"] == (300, 0, 0)
    assert [r[1:] for r in below][::11] == [(158334975, 1), (2051014653, 12)]
    assert at_limit == [(327, INT_MAX, 13)] and [s["estimate"] for s in silent] == [(330, 14, INT_MAX)]
    _, _, segs = shapes._case_large_vertices(10 ** 6 + 3, False)
    below, at_limit, silent = shapes._row_facts(segs[1:])
    assert len(below) == 14 and not at_limit and not silent
    src, dst, segs = shapes._case_large_vertices(10 ** 6 + 3, True, every=64)
    assert min(src.min(), dst.min()) < 0 and max(src.max(), dst.max()) > 1 << 62


def test_late_edge_counts_end_at_the_arrival_limit_without_a_resample():
    (psrc, _, pre), (src, _, late) = shapes._case_late_edge_counts()
    assert len(psrc) == 40 and pre["estimate"] == (40, 0, 0) and pre["coins"] >= 4096
    below, at_limit, silent = shapes._row_facts(late)
    assert len(src) == 200 and len(below) >= 8 and len(at_limit) == 1 and len(silent) >= 1
    assert below[0][0] > INT_MAX - 200 and at_limit[0][2] > 512 >= below[-1][2]
    assert sum(s["coins"] for s in late) == 0 and late[-1]["estimate"][::2] == (INT_MAX, INT_MAX)


def test_pieces_and_coin_flushes():
    for samples, n, piece, seed in ((65, 3 * 1024 + 5, 16, 51), (65, 3 * 1024 + 5, 1024, 51), (300, 77, 16, 7)):
        src, dst, (main, tail) = shapes._case_pieces(samples, n, piece, seed)
        assert main["pieces"] == -(-n // piece) and (main["lo"], main["hi"], tail["hi"]) == (0, n, len(src))
        assert tail["hi"] - tail["lo"] <= piece and len(src) >= 77
        model = Model(samples, 6)  # the sums over the pieces are the whole fold's
        rows = model.fold(src[:n].tolist(), dst[:n].tolist())
        assert (rows, model.coins, model.max_attempts) == (main["rows"], main["coins"], main["max_attempts"])
    src, dst = shapes._case_coin_flushes()
    model = Model(64, 6)
    model.fold(src.tolist(), dst.tolist())
    assert len(src) == 2000 and model.coins == 528 > 2 * shapes.COIN_FLUSH
    # a model of 64 samples is the first 64 instances of a larger one
    wide = Model(300, 6)
    wide.fold(src[:50].tolist(), dst[:50].tolist())
    narrow = Model(64, 6)
    narrow.fold(src[:50].tolist(), dst[:50].tolist())
    assert wide.states()[:64] == narrow.states()
    assert _dense_stream(6, 2000, 61)[0].tolist() == src.tolist()
