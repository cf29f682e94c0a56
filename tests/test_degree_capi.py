"""CPU: the degree summary's entry points exist, are declared in gs_summary.h, exported and
bound, and reject null arguments before touching a device. No compute calls here (the
results are checked on the GPU in test_gpu_degrees.py)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_degree_fold", "gs_degree_fold_device", "gs_degree_find_device", "gs_degree_export_device",
         "gs_degree_export", "gs_degree_distribution_device", "gs_degree_distribution")


def test_names_are_declared_exported_and_bound(gs):
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    L = gs.lib()
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert re.search(r"\bint %s\(gs_handle h," % n, text), n
        assert getattr(L, n).argtypes, n
    assert re.search(r"GS_KIND_DEGREE = 2\b", text)
    assert re.search(r"GS_DEGREE_ALL = 0, GS_DEGREE_IN = 1, GS_DEGREE_OUT = 2", text)
    assert (gs.KIND_DEGREE, gs.DEGREE_ALL, gs.DEGREE_IN, gs.DEGREE_OUT) == (2, 0, 1, 2)


def test_null_handle_is_rejected(gs):
    L = gs.lib()
    n = ctypes.c_size_t(7)
    calls = (
        lambda: L.gs_degree_fold(None, None, None, None, 0, 0),
        lambda: L.gs_degree_fold_device(None, None, None, None, 0, 1, 0),
        lambda: L.gs_degree_find_device(None, None, 0, None, None),
        lambda: L.gs_degree_export_device(None, None, None, 0, ctypes.byref(n), 0),
        lambda: L.gs_degree_export(None, None, None, 0, ctypes.byref(n), 1),
        lambda: L.gs_degree_distribution_device(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_degree_distribution(None, None, None, 0, ctypes.byref(n)),
    )
    for c in calls:
        assert c() == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()


def test_null_counts_are_rejected(gs):
    L = gs.lib()
    assert L.gs_degree_export_device(None, None, None, 0, None, 0) == gs.GS_ERR_INVALID
    assert L.gs_degree_export(None, None, None, 0, None, 0) == gs.GS_ERR_INVALID
    assert L.gs_degree_distribution_device(None, None, None, 0, None) == gs.GS_ERR_INVALID
    assert L.gs_degree_distribution(None, None, None, 0, None) == gs.GS_ERR_INVALID


def test_python_class_has_the_methods(gs):
    for m in ("fold", "fold_device", "find_device", "degrees", "degrees_device", "distribution",
              "distribution_device", "combine", "serialize", "deserialize", "reset", "sync", "num_vertices",
              "close", "__enter__", "__exit__"):
        assert callable(getattr(gs.Degrees, m)), m
    assert isinstance(gs.Degrees.stream, property)
    assert set(gs.Degrees.DIRECTIONS) == {"all", "in", "out"}


def test_degree_tile_constant_matches_the_kernels(gs):
    """gsamd.DEGREE_TILE (the sizes test_gpu_degrees.py brackets) is the kernel header's
    DEGREE_TILE = threads x edges per thread."""
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_degree.hpp")) as f:
        text = f.read()
    tile = int(re.search(r"constexpr uint32_t DEGREE_TILE = (\d+);", text).group(1))
    bs = int(re.search(r"kDegreeBS = (\d+);", text).group(1))
    items = int(re.search(r"kDegreeItems = (\d+);", text).group(1))
    assert gs.DEGREE_TILE == tile == bs * items


def test_create_bytes_accepts_the_degree_kind(gs):
    b = ctypes.c_uint64(0)
    assert gs.lib().gs_create_bytes(2, 1 << 10, ctypes.byref(b)) == gs.GS_OK
    assert b.value > 0
    assert gs.create_bytes("degree", 1 << 10) == b.value == gs.create_bytes("cc", 1 << 10)
    assert gs.lib().gs_create_bytes(3, 1 << 10, ctypes.byref(b)) == gs.GS_ERR_INVALID


def test_degree_variant_knob_roundtrip(gs):
    assert gs.testing_get("degree_variant") == 0
    with gs.testing(degree_variant=1):
        assert gs.testing_get("degree_variant") == 1
    assert gs.testing_get("degree_variant") == 0


def test_fixture_is_data_with_citations():
    with open(os.path.join(ROOT, "tests", "golden", "degree_pins.json")) as f:
        pins = json.load(f)
    for k in ("sample_edges", "get_degrees", "get_in_degrees", "get_out_degrees", "degrees_data", "degrees_result",
              "degrees_data_zero", "degrees_result_zero"):
        assert ".java:" in pins[k]["cite"], k
    assert len(pins["sample_edges"]["edges"]) == 7
