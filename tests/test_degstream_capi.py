"""CPU: the degree streams' entry points exist, are declared in gs_summary.h, exported and bound,
and reject null arguments before touching a device. No compute calls here (the results are
checked on the GPU in test_gpu_degstream.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_degstream_create", "gs_degstream_destroy", "gs_degstream_reset", "gs_degstream_fold",
         "gs_degstream_fold_device", "gs_degstream_rows", "gs_degstream_rows_device", "gs_degstream_records",
         "gs_degstream_records_device", "gs_degstream_size", "gs_degstream_degrees", "gs_degstream_degrees_device",
         "gs_degstream_distribution", "gs_degstream_distribution_device", "gs_degstream_sync",
         "gs_degstream_get_stream", "gs_degstream_wait_stream")
TESTING = ("gs_testing_degstream_stats", "gs_testing_degstream_tune")


def test_names_are_declared_exported_and_bound(gs):
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    L = gs.lib()
    assert re.search(r"typedef struct gs_degstream_s\* gs_degstream;", text)
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert not re.search(r"\d", n)
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert re.search(r"\bint %s\(gs_degstream\*? \w+[,)]" % n, text), n
        assert getattr(L, n).argtypes, n
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    for n in TESTING:
        assert n in gs.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert getattr(L, n).argtypes
    assert re.search(r"\bint gs_testing_degstream_stats\(void\* d, uint64_t\* out\);", testing)
    assert re.search(r"\bint gs_testing_degstream_tune\(void\* d, int what, int64_t value\);", testing)
    # the header states the rule, the overflow rule, the largest fold with rows, and what is not built
    for phrase in ("new = max(d + c, 0)", "(new, +1) if new > 0, then (old, -1)", "old == 0 and c < 0: none",
                   "past 2^31 - 1 fails with GS_ERR_CAPACITY before any work",
                   "The largest fold whose rows are kept has 2^24", "however the stream is cut",
                   "Not built: combine, serialization, multi-GPU groups, parallelism above 1"):
        assert phrase in text, phrase


def test_null_handles_and_pointers_are_rejected(gs):
    L = gs.lib()
    n = ctypes.c_size_t(7)
    w = (ctypes.c_uint64 * 9)()
    p = ctypes.c_void_p()
    calls = (
        lambda: L.gs_degstream_create(None, 0, 0, 16),
        lambda: L.gs_degstream_reset(None),
        lambda: L.gs_degstream_fold(None, None, None, None, 0),
        lambda: L.gs_degstream_fold_device(None, None, None, None, 0, 1),
        lambda: L.gs_degstream_rows(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degstream_rows_device(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degstream_records(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degstream_records_device(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degstream_size(None, w),
        lambda: L.gs_degstream_degrees(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degstream_degrees_device(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degstream_distribution(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degstream_distribution_device(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degstream_sync(None),
        lambda: L.gs_degstream_get_stream(None, ctypes.byref(p)),
        lambda: L.gs_degstream_wait_stream(None, None),
        lambda: L.gs_testing_degstream_stats(None, w),
        lambda: L.gs_testing_degstream_tune(None, 0, 1),
    )
    for c in calls:
        assert c() == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()
    assert L.gs_degstream_destroy(None) == gs.GS_OK
    assert n.value == 7


def test_python_class_has_the_methods(gs):
    for m in ("close", "reset", "sync", "wait_stream", "fold", "fold_device", "rows", "rows_device", "records",
              "records_device", "degrees", "degrees_device", "distribution", "distribution_device", "size", "stats",
              "phases", "tune",
              "__enter__", "__exit__"):
        assert callable(getattr(gs.DegreeStream, m)), m
    assert isinstance(gs.DegreeStream.stream, property)
    assert issubclass(gs.DegreeStream, gs._Handle)
    assert "__del__" not in vars(gs.DegreeStream) and "close" not in vars(gs.DegreeStream)
    assert gs.DegreeStream.DIRECTIONS == gs.Degrees.DIRECTIONS


def test_degstream_constants_match_the_headers(gs):
    csrc = os.path.join(ROOT, "gelly-streaming_amd", "csrc")
    with open(os.path.join(csrc, "gs_degstream_seq.hpp")) as f:
        seq = f.read()
    with open(os.path.join(csrc, "gs_degstream.hpp")) as f:
        hpp = f.read()
    assert gs.DEGSTREAM_TILE == int(re.search(r"constexpr uint32_t DEGSTREAM_TILE = (\d+);", hpp).group(1))
    assert gs.DEGSTREAM_MIN_COUNTS == int(re.search(r"constexpr uint64_t kDsMinCounts = (\d+);", hpp).group(1))
    assert gs.DEGSTREAM_MAX_TOTAL == int(re.search(r"constexpr uint64_t kDsMaxTotal = (0x[0-9A-F]+)ull;", seq).group(1), 16)
    assert gs.DEGSTREAM_MAX_FOLD == 1 << int(re.search(r"constexpr uint64_t kDsMaxFold = 1ull << (\d+);", seq).group(1))
    assert re.search(r"enum DsDirection : int \{ kDsAll = 0, kDsIn = 1, kDsOut = 2, kDsDirections = 3 \};", seq)
    assert (gs.DEGREE_ALL, gs.DEGREE_IN, gs.DEGREE_OUT) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        assert "first\n * capacity: %d" % gs.DEGSTREAM_MIN_COUNTS in f.read()
    with open(os.path.join(ROOT, "gelly-streaming_amd", "Makefile")) as f:
        mk = f.read()
    for name in ("csrc/gs_degstream.hpp", "csrc/gs_degstream_seq.hpp", "gs_degstream_k.o", "gs_degstream.o"):
        assert name in mk, name
