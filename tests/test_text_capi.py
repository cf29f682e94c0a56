"""CPU: the C ABI of the field-spec text ingest and the text reader (include/gs_ingest.h): the
symbols are exported, null and invalid arguments are refused before any device call, nothing
runs without a GPU, and TextReader.fold_into refuses a target its third field does not fit before
it touches a device."""
import ctypes
import os

import pytest

SYMBOLS = ("gs_parse_records_device", "gs_window_bounds_device", "gs_text_create", "gs_text_destroy",
           "gs_text_set_window", "gs_text_open", "gs_text_next", "gs_text_windows", "gs_text_position", "gs_text_sync",
           "gs_text_get_stream", "gs_text_wait_stream", "gs_testing_text_stats")


def test_symbols_are_exported(gs):
    L = ctypes.CDLL(gs.LIB_PATH)
    assert not [n for n in SYMBOLS if not hasattr(L, n)]
    assert set(SYMBOLS) <= set(gs.EXPORTED_SYMBOLS)
    assert (gs.TEXT_THIRD, gs.TEXT_INT32, gs.TEXT_COMMENT_PERCENT) == ({None: 0, "long": 1, "event": 2}, 1, 2)


def test_null_and_invalid_arguments_are_refused(gs):
    L = gs.lib()
    n, r, w = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    bad = ctypes.c_int64()
    out = (ctypes.c_int64 * 4)()
    R = ctypes.byref
    text = b"1 2 3\n"

    def parse(sep=0, third=0, flags=0, src=out, dst=out, val=None, dele=None, cap=1, nl=R(n), nr=R(r), b=R(bad),
              t=text, ln=len(text)):
        return L.gs_parse_records_device(None, t, ln, sep, third, flags, src, dst, val, dele, cap, nl, nr, b)

    for kw in (dict(nl=None), dict(nr=None), dict(b=None), dict(t=None), dict(sep=2), dict(sep=-1), dict(third=3),
               dict(third=-1), dict(flags=4), dict(flags=-1), dict(third=1), dict(third=2), dict(src=None),
               dict(dst=None), dict(third=1, dele=out), dict(third=2, val=out)):
        assert parse(**kw) == gs.GS_ERR_INVALID, kw
    # an empty text is no work: GS_OK without a device
    assert parse(t=None, ln=0, third=1, val=out) == gs.GS_OK and (n.value, r.value, bad.value) == (0, 0, -1)

    def bounds(ts=out, n_=1, size=10, first=out, window=out, cap=1, nw=R(w)):
        return L.gs_window_bounds_device(None, ts, n_, size, first, window, cap, nw)

    for kw in (dict(nw=None), dict(size=0), dict(size=-5), dict(ts=None), dict(first=None), dict(window=None)):
        assert bounds(**kw) == gs.GS_ERR_INVALID, kw
    assert bounds(ts=None, n_=0) == gs.GS_OK and w.value == 0

    h = ctypes.c_void_p()
    assert L.gs_text_create(None, 0, 0, 0, 0, 0) == gs.GS_ERR_INVALID
    for sep, third, flags, chunk in ((2, 0, 0, 0), (0, 3, 0, 0), (0, 0, 4, 0), (0, 0, 0, (1 << 30) + 1)):
        assert L.gs_text_create(R(h), 0, sep, third, flags, chunk) == gs.GS_ERR_INVALID and not h.value
    assert b"text reader" in L.gs_last_error()
    assert L.gs_text_destroy(None) == gs.GS_OK
    p = ctypes.c_void_p()
    k, last = ctypes.c_size_t(), ctypes.c_int()
    assert L.gs_text_next(None, R(p), R(p), None, None, R(k), None, None, None, R(last)) == gs.GS_ERR_INVALID
    assert b"null text reader handle" in L.gs_last_error()
    for call in (lambda: L.gs_text_set_window(None, 10), lambda: L.gs_text_open(None, text, len(text)),
                 lambda: L.gs_text_position(None, None, None, None), lambda: L.gs_text_windows(None, None, None, 0, R(k)), lambda: L.gs_text_sync(None),
                 lambda: L.gs_text_get_stream(None, R(p)), lambda: L.gs_text_wait_stream(None, None)):
        assert call() == gs.GS_ERR_INVALID
    assert L.gs_testing_text_stats(None) == gs.GS_ERR_INVALID
    for third in ("float", 1, "LONG"):
        with pytest.raises(ValueError):
            gs.TextReader(third=third)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_gpu_fails_loudly(gs):
    with pytest.raises(gs.GSError) as e:
        gs.TextReader(third="long")
    assert e.value.code == gs.GS_ERR_HIP
    L = gs.lib()
    n, r, bad = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int64()
    out = (ctypes.c_int64 * 4)()
    rc = L.gs_parse_records_device(None, b"1 2 3\n", 6, 0, 1, 0, out, out, out, None, 1, ctypes.byref(n), ctypes.byref(r),
                                   ctypes.byref(bad))
    assert rc == gs.GS_ERR_HIP
    w = ctypes.c_uint64()
    assert L.gs_window_bounds_device(None, out, 4, 10, out, out, 4, ctypes.byref(w)) == gs.GS_ERR_HIP


def test_fold_into_refuses_a_mismatch_before_any_device_call(gs):
    """Degrees / DegreeStream take an 'event' reader or one without a third field, Matching a
    'long' one, every other handle one without a third field. The objects hold no handle: a
    dispatch that reached a fold or the reader would fail otherwise than with ValueError."""
    def bare(cls, **attrs):
        o = cls.__new__(cls)
        o._h = None
        for k, v in attrs.items():
            setattr(o, k, v)
        return o

    plain = (gs.Summary, gs.Triangles, gs.SlidingTriangles, gs.TriangleStream, gs.Distinct, gs.Spanner,
             gs.TriangleSampler)
    fits = {None: plain + (gs.Degrees, gs.DegreeStream), "event": (gs.Degrees, gs.DegreeStream), "long": (gs.Matching,)}
    for third in (None, "long", "event"):
        reader = bare(gs.TextReader, third=third, device=0)
        for cls in plain + (gs.Degrees, gs.DegreeStream, gs.Matching):
            if cls in fits[third]:
                assert reader._fold_kind(bare(cls)) in ("plain", "deletions", "val")
                continue
            with pytest.raises(ValueError):
                reader.fold_into(bare(cls), b"1 2 3\n")
        with pytest.raises(ValueError):
            reader.fold_into(object(), b"1 2\n")
    assert bare(gs.TextReader, third="event")._fold_kind(bare(gs.DegreeStream)) == "deletions"
    assert bare(gs.TextReader, third="long")._fold_kind(bare(gs.Matching)) == "val"
    with pytest.raises(ValueError):
        next(bare(gs.TextReader, third=None).windows(b"1 2 3\n", 10))
