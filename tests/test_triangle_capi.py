"""CPU: the triangle summary's entry points exist, are declared in gs_summary.h, exported and
bound, and reject null arguments before touching a device. No compute calls here (the
results are checked on the GPU in test_gpu_triangles.py)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_triangle_create", "gs_triangle_destroy", "gs_triangle_reset", "gs_triangle_fold",
         "gs_triangle_fold_device", "gs_triangle_count", "gs_triangle_count_device", "gs_triangle_find_device",
         "gs_triangle_export_device", "gs_triangle_export", "gs_triangle_sync", "gs_triangle_get_stream",
         "gs_triangle_wait_stream")


def test_names_are_declared_exported_and_bound(gs):
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    L = gs.lib()
    assert re.search(r"typedef struct gs_triangles_s\* gs_triangles;", text)
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert not re.search(r"\d", n)
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert re.search(r"\bint %s\(gs_triangles\*? \w+[,)]" % n, text), n
        assert getattr(L, n).argtypes, n
    assert "gs_testing_triangle_stats" in gs.EXPORTED_SYMBOLS
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    for n in ("gs_testing_triangle_stats", "gs_testing_triangle_bins"):
        assert n in gs.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert re.search(r"\bint %s\(void\* t, uint64_t\* out\);" % n, testing), n
        assert getattr(L, n).argtypes, n


def test_null_handles_and_pointers_are_rejected(gs):
    L = gs.lib()
    n = ctypes.c_size_t(7)
    w = ctypes.c_uint64(0)
    p = ctypes.c_void_p()
    calls = (
        lambda: L.gs_triangle_create(None, 0, 16),
        lambda: L.gs_triangle_reset(None),
        lambda: L.gs_triangle_fold(None, None, None, 0),
        lambda: L.gs_triangle_fold_device(None, None, None, 0, 1),
        lambda: L.gs_triangle_count(None, ctypes.byref(w), ctypes.byref(w), ctypes.byref(w)),
        lambda: L.gs_triangle_count_device(None, None),
        lambda: L.gs_triangle_find_device(None, None, 0, None, None),
        lambda: L.gs_triangle_export_device(None, None, None, 0, ctypes.byref(n), 0),
        lambda: L.gs_triangle_export(None, None, None, 0, ctypes.byref(n), 1),
        lambda: L.gs_triangle_sync(None),
        lambda: L.gs_triangle_get_stream(None, ctypes.byref(p)),
        lambda: L.gs_triangle_wait_stream(None, None),
        lambda: L.gs_testing_triangle_stats(None, ctypes.byref(w)),
        lambda: L.gs_testing_triangle_bins(None, ctypes.byref(w)),
    )
    for c in calls:
        assert c() == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()
    assert L.gs_triangle_destroy(None) == gs.GS_OK


def test_python_class_has_the_methods(gs):
    for m in ("close", "reset", "sync", "wait_stream", "fold", "fold_device", "count", "count_device", "find_device",
              "local_counts", "local_counts_device", "window", "stats", "bins", "__enter__", "__exit__"):
        assert callable(getattr(gs.Triangles, m)), m
    assert isinstance(gs.Triangles.stream, property)


def test_triangle_constants_match_the_kernels(gs):
    """gsamd.TRIANGLE_LANES / TRIANGLE_TILE (the sizes test_gpu_triangles.py brackets) are the
    kernel header's: the lane group of the product's short bin, and threads x elements per
    thread of the per-edge passes."""
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_triangle.hpp")) as f:
        text = f.read()
    lanes = int(re.search(r"constexpr uint32_t TRIANGLE_LANES = (\d+);", text).group(1))
    tile = int(re.search(r"constexpr uint32_t TRIANGLE_TILE = (\d+);", text).group(1))
    bs = int(re.search(r"constexpr uint32_t kTriBS = (\d+);", text).group(1))
    variants = int(re.search(r"kTriangleVariants = (\d+),", text).group(1))
    assert re.search(r"kTriPer = TRIANGLE_TILE / kTriBS;", text) and tile % bs == 0
    assert gs.TRIANGLE_LANES == lanes and gs.TRIANGLE_TILE == tile and gs.TRIANGLE_VARIANTS == variants
    assert re.search(r"kTriangleProduct = kTriangleBinned\b", text) and re.search(r"kTriangleBinned = 0,", text)
    # the bins of the product's count step, whose thresholds test_gpu_triangles.py brackets
    assert re.search(r"constexpr uint32_t kTriShortRow = 4 \* TRIANGLE_LANES;", text)
    wave = int(re.search(r"constexpr uint32_t kTriWaveRow = (\d+);", text).group(1))
    lds = int(re.search(r"constexpr uint32_t kTriLdsRow = (\d+);", text).group(1))
    samples = int(re.search(r"constexpr uint32_t kTriSamples = (\d+);", text).group(1))
    assert gs.TRIANGLE_SHORT_ROW == 4 * lanes and gs.TRIANGLE_WAVE_ROW == wave
    assert gs.TRIANGLE_LDS_ROW == lds and gs.TRIANGLE_SAMPLES == samples
    assert gs.TRIANGLE_SHORT_ROW < gs.TRIANGLE_WAVE_ROW < gs.TRIANGLE_SAMPLES <= gs.TRIANGLE_LDS_ROW


def test_triangle_variant_knob_roundtrip(gs):
    assert gs.testing_get("triangle_variant") == 0
    with gs.testing(triangle_variant=1):
        assert gs.testing_get("triangle_variant") == 1
    assert gs.testing_get("triangle_variant") == 0


def test_fixture_is_data_with_citations():
    with open(os.path.join(ROOT, "tests", "golden", "triangle_pins.json")) as f:
        pins = json.load(f)
    for k in ("triangles_data", "triangles_result", "exact_default_stream", "exact_default_counters"):
        assert ".java:" in pins[k]["cite"], k
    assert len(pins["triangles_data"]["edges"]) == 19
    assert len(pins["exact_default_stream"]["edges"]) == 9
    assert sorted(pins["triangles_result"]["rows"]) == [[2, 399], [2, 1199], [3, 799]]
