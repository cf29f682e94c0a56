"""CPU: the window slices' entry points exist, are declared in gs_summary.h, exported and bound,
and reject null arguments before touching a device. No compute calls here (the results are
checked on the GPU in test_gpu_slice.py)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_slice_create", "gs_slice_destroy", "gs_slice_window", "gs_slice_window_device", "gs_slice_size",
         "gs_slice_reduce_device", "gs_slice_reduce", "gs_slice_neighborhoods_device", "gs_slice_neighborhoods",
         "gs_slice_sync", "gs_slice_get_stream", "gs_slice_wait_stream")


def test_names_are_declared_exported_and_bound(gs):
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    L = gs.lib()
    assert re.search(r"typedef struct gs_slices_s\* gs_slices;", text)
    assert re.search(r"enum gs_slice_dir \{ GS_SLICE_OUT = 0, GS_SLICE_IN = 1, GS_SLICE_ALL = 2 \};", text)
    assert re.search(r"enum gs_slice_op \{ GS_SLICE_SUM = 0, GS_SLICE_MIN = 1, GS_SLICE_MAX = 2, GS_SLICE_COUNT = 3 \};",
                     text)
    assert gs.SLICE_DIRECTIONS == {"out": 0, "in": 1, "all": 2}
    assert gs.SLICE_OPS == {"sum": 0, "min": 1, "max": 2, "count": 3}
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert not re.search(r"\d", n)
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert re.search(r"\bint %s\(gs_slices\*? \w+[,)]" % n, text), n
        assert getattr(L, n).argtypes, n
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    assert "gs_testing_slice_stats" in gs.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(gs.LIB_PATH), "gs_testing_slice_stats")
    assert re.search(r"\bint gs_testing_slice_stats\(void\* s, uint64_t\* out\);", testing)
    assert L.gs_testing_slice_stats.argtypes


def test_null_handles_and_pointers_are_rejected(gs):
    L = gs.lib()
    n = ctypes.c_size_t(7)
    w = ctypes.c_uint64(0)
    p = ctypes.c_void_p()
    calls = (
        lambda: L.gs_slice_create(None, 0, 16),
        lambda: L.gs_slice_window(None, None, None, None, 0, 0),
        lambda: L.gs_slice_window_device(None, None, None, None, 0, 1, 0),
        lambda: L.gs_slice_size(None, ctypes.byref(w), ctypes.byref(w)),
        lambda: L.gs_slice_reduce_device(None, 0, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_slice_reduce(None, 3, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_slice_neighborhoods_device(None, None, None, None, None, 0, 0, ctypes.byref(n), ctypes.byref(n)),
        lambda: L.gs_slice_neighborhoods(None, None, None, None, None, 0, 0, ctypes.byref(n), ctypes.byref(n)),
        lambda: L.gs_slice_sync(None),
        lambda: L.gs_slice_get_stream(None, ctypes.byref(p)),
        lambda: L.gs_slice_wait_stream(None, None),
        lambda: L.gs_testing_slice_stats(None, ctypes.byref(w)),
    )
    for c in calls:
        assert c() == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()
    assert L.gs_slice_destroy(None) == gs.GS_OK


def test_python_class_has_the_methods(gs):
    for m in ("close", "sync", "wait_stream", "window", "window_device", "size", "reduce", "reduce_device",
              "neighborhoods", "neighborhoods_device", "stats", "__enter__", "__exit__"):
        assert callable(getattr(gs.Slice, m)), m
    assert isinstance(gs.Slice.stream, property)


def test_slice_tile_matches_the_kernels(gs):
    """gsamd.SLICE_TILE (the size test_gpu_slice.py brackets) is the kernel header's: threads x
    consecutive positions per thread of the heads and reduce kernels."""
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_slice.hpp")) as f:
        text = f.read()
    tile = int(re.search(r"constexpr uint32_t SLICE_TILE = (\d+);", text).group(1))
    bs = int(re.search(r"constexpr uint32_t kSliceBS = (\d+);", text).group(1))
    assert re.search(r"kSlicePer = SLICE_TILE / kSliceBS;", text) and tile % bs == 0
    assert gs.SLICE_TILE == tile and bs == 256


def test_slice_profile_knob_roundtrip(gs):
    assert gs.testing_get("slice_profile") == 0
    with gs.testing(slice_profile=1):
        assert gs.testing_get("slice_profile") == 1
    assert gs.testing_get("slice_profile") == 0


def test_fixture_is_data_with_citations():
    with open(os.path.join(ROOT, "tests", "golden", "slice_pins.json")) as f:
        pins = json.load(f)
    assert "GraphStreamTestUtils.java:" in pins["edges"]["cite"] and len(pins["edges"]["rows"]) == 7
    assert "TestSlice.java:" in pins["threshold"]["cite"] and pins["threshold"]["value"] == 50
    for k in ("sum_out", "sum_in", "sum_all", "apply_out", "apply_in", "apply_all"):
        assert "TestSlice.java:" in pins[k]["cite"], k
        assert [r[0] for r in pins[k]["rows"]] == [1, 2, 3, 4, 5], k
    assert [r[1] for r in pins["sum_all"]["rows"]] == [76, 35, 105, 79, 131]
    # the fixture against itself: ALL is OUT plus IN
    for o, i, a in zip(pins["sum_out"]["rows"], pins["sum_in"]["rows"], pins["sum_all"]["rows"]):
        assert o[1] + i[1] == a[1]
