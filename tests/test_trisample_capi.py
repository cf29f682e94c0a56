"""CPU: the sampling triangle estimate's entry points exist, are declared in gs_summary.h, exported
and bound, reject null arguments and the limits of create before touching a device. No compute
calls here (the results are checked on the GPU in test_gpu_trisample.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_trisample_create", "gs_trisample_destroy", "gs_trisample_reset", "gs_trisample_fold",
         "gs_trisample_fold_device", "gs_trisample_rows", "gs_trisample_rows_device", "gs_trisample_estimate",
         "gs_trisample_states", "gs_trisample_states_device", "gs_trisample_sync", "gs_trisample_get_stream",
         "gs_trisample_wait_stream")
TESTING = ("gs_testing_trisample_stats", "gs_testing_trisample_tune")


def test_names_are_declared_exported_and_bound(gs):
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    L = gs.lib()
    assert re.search(r"typedef struct gs_trisample_s\* gs_trisample;", text)
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert not re.search(r"\d", n)
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert re.search(r"\bint %s\(gs_trisample\*? \w+[,)]" % n, text), n
        assert getattr(L, n).argtypes, n
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    for n in TESTING:
        assert n in gs.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert getattr(L, n).argtypes
    assert re.search(r"\bint gs_testing_trisample_stats\(void\* t, uint64_t\* out\);", testing)
    assert re.search(r"\bint gs_testing_trisample_tune\(void\* t, int what, int64_t value\);", testing)
    # the header states the contract, what is this project's own and what is not built
    for phrase in ("nextDouble() * (double)t <= 1.0", "it is always true at t = 1", "unseeded Math.random()",
                   "0x9E3779B97F4A7C15", "truncate, saturate, NaN -> 0", "does not depend on where it is cut",
                   "Not built: parallelism above 1", "IncidenceSampling's intermediate emissions",
                   "combine, serialization, multi-GPU groups"):
        assert phrase in text, phrase


def test_null_handles_and_pointers_are_rejected(gs):
    L = gs.lib()
    n = ctypes.c_size_t(7)
    w = ctypes.c_uint64(0)
    i = ctypes.c_int32(0)
    p = ctypes.c_void_p()
    calls = (
        lambda: L.gs_trisample_create(None, 0, 16, 16, 0, 0),
        lambda: L.gs_trisample_reset(None),
        lambda: L.gs_trisample_fold(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_trisample_fold_device(None, None, None, 0, 1, ctypes.byref(n)),
        lambda: L.gs_trisample_rows(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_trisample_rows_device(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_trisample_estimate(None, ctypes.byref(w), ctypes.byref(i), ctypes.byref(i)),
        lambda: L.gs_trisample_states(None, None, None, None, None, None),
        lambda: L.gs_trisample_states_device(None, None, None, None, None, None),
        lambda: L.gs_trisample_sync(None),
        lambda: L.gs_trisample_get_stream(None, ctypes.byref(p)),
        lambda: L.gs_trisample_wait_stream(None, None),
        lambda: L.gs_testing_trisample_stats(None, ctypes.byref(w)),
        lambda: L.gs_testing_trisample_tune(None, 0, 1),
    )
    for c in calls:
        assert c() == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()
    assert L.gs_trisample_destroy(None) == gs.GS_OK
    assert n.value == 7


def test_limits_of_create_are_rejected_before_a_device_is_touched(gs):
    L = gs.lib()
    for samples, vertices, word in ((0, 1000, b"samples"), ((1 << 20) + 1, 1000, b"samples"), (1 << 63, 1000, b"samples"),
                                    (100, 2, b"vertices"), (100, 0, b"vertices"), (100, -7, b"vertices"),
                                    (100, 1 << 31, b"vertices"), (100, 1 << 40, b"vertices")):
        h = ctypes.c_void_p(12345)
        assert L.gs_trisample_create(ctypes.byref(h), 0, samples, vertices, gs.TRISAMPLE_SEED, 0) == gs.GS_ERR_INVALID
        assert word in L.gs_last_error(), (samples, vertices)
        assert not h.value  # no handle
    # (the limit of 2^31 - 1 arrivals in total needs a handle: test_gpu_trisample.py)


def test_python_class_has_the_methods(gs):
    for m in ("close", "reset", "sync", "wait_stream", "fold", "fold_device", "rows", "rows_device", "estimate",
              "states", "states_device", "stats", "tune", "__enter__", "__exit__"):
        assert callable(getattr(gs.TriangleSampler, m)), m
    assert isinstance(gs.TriangleSampler.stream, property)
    assert issubclass(gs.TriangleSampler, gs._Handle)
    assert "__del__" not in vars(gs.TriangleSampler) and "close" not in vars(gs.TriangleSampler)
    import inspect
    assert str(inspect.signature(gs.TriangleSampler.__init__)) == \
        "(self, samples=10000, vertices=1000, seed=-559038737, third_seed=0, device=0)"
    assert str(inspect.signature(gs.TriangleSampler.tune)) == \
        "(self, chunk=None, tile=None, profile=None, keys=None, piece=None, edge_count=None)"


def test_tune_rejects_an_unknown_control_and_an_edge_count_out_of_range(gs):
    """The controls are 0..5 (include/gs_testing.h); edge_count (5) takes 0 .. 2^31 - 1. The
    arguments are checked before the handle, so this needs no device; a valid control on a null
    handle still names the handle."""
    L = gs.lib()
    for what, value, word in ((6, 1, b"unknown control"), (-1, 1, b"unknown control"),
                              (5, -1, b"edge_count"), (5, 1 << 31, b"edge_count")):
        assert L.gs_testing_trisample_tune(None, what, value) == gs.GS_ERR_INVALID
        assert word in L.gs_last_error(), (what, value)
    for what, value in ((4, 16), (5, 0), (5, gs.TRISAMPLE_MAX_ARRIVALS)):
        assert L.gs_testing_trisample_tune(None, what, value) == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error(), (what, value)
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    for phrase in ("what = 4 piece", "what = 5 edge_count is an action", "NO real stream",
                   "gs_testing_spanner_generation does"):
        assert phrase in testing, phrase


def test_trisample_constants_match_the_headers(gs):
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_trisample_seq.hpp")) as f:
        seq = f.read()
    assert gs.TRISAMPLE_CHUNK == int(re.search(r"constexpr uint32_t kTsChunk = (\d+);", seq).group(1))
    assert gs.TRISAMPLE_TILE == int(re.search(r"constexpr uint32_t kTsTile = (\d+);", seq).group(1))
    assert gs.TRISAMPLE_MAX_SAMPLES == 1 << int(re.search(r"constexpr uint32_t kTsMaxSamples = 1u << (\d+);", seq).group(1))
    assert gs.TRISAMPLE_MAX_VERTICES == int(re.search(r"constexpr int64_t kTsMaxVertices = (\d+);", seq).group(1))
    assert gs.TRISAMPLE_MAX_ARRIVALS == int(re.search(r"constexpr uint64_t kTsMaxArrivals = (\d+);", seq).group(1))
    assert gs.TRISAMPLE_SEED == int(re.search(r"constexpr int64_t kTsDefaultSeed = (-\d+);", seq).group(1))
    assert gs.TRISAMPLE_SEED == 0xDEADBEEF - (1 << 32)
    assert gs.TRISAMPLE_MAX_FOLD == 1 << int(re.search(r"constexpr uint64_t kTsMaxFold = 1ull << (\d+);", seq).group(1))
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    assert "(product: %d)" % gs.TRISAMPLE_CHUNK in testing and "(product: %d," % gs.TRISAMPLE_TILE in testing
