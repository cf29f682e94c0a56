"""CPU: the k-spanner summary's entry points exist, are declared in gs_summary.h, exported and
bound, and reject null arguments and a k outside 1..16 before touching a device. No compute calls
here (the results are checked on the GPU in test_gpu_spanner.py)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_spanner_create", "gs_spanner_destroy", "gs_spanner_reset", "gs_spanner_fold", "gs_spanner_fold_device",
         "gs_spanner_add", "gs_spanner_within", "gs_spanner_within_device", "gs_spanner_combine", "gs_spanner_count",
         "gs_spanner_export_device", "gs_spanner_export", "gs_spanner_neighbors", "gs_spanner_sync",
         "gs_spanner_get_stream", "gs_spanner_wait_stream")


def test_names_are_declared_exported_and_bound(gs):
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    L = gs.lib()
    assert re.search(r"typedef struct gs_spanner_s\* gs_spanner;", text)
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert not re.search(r"\d", n)
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert re.search(r"\bint %s\(gs_spanner\*? \w+[,)]" % n, text), n
        assert getattr(L, n).argtypes, n
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    n = "gs_testing_spanner_stats"
    assert n in gs.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(gs.LIB_PATH), n)
    assert re.search(r"\bint %s\(void\* s, uint64_t\* out\);" % n, testing)
    assert getattr(L, n).argtypes
    n = "gs_testing_spanner_generation"
    assert n in gs.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(gs.LIB_PATH), n)
    assert re.search(r"\bint %s\(void\* s, int64_t set, uint64_t\* out\);" % n, testing)
    assert getattr(L, n).argtypes
    # the header says which k is rejected
    assert "1 <= k <= 16; any other k returns GS_ERR_INVALID" in text


def test_null_handles_and_pointers_are_rejected(gs):
    L = gs.lib()
    n = ctypes.c_size_t(7)
    w = ctypes.c_uint64(0)
    p = ctypes.c_void_p()
    calls = (
        lambda: L.gs_spanner_create(None, 0, 3, 16),
        lambda: L.gs_spanner_reset(None),
        lambda: L.gs_spanner_fold(None, None, None, 0, None),
        lambda: L.gs_spanner_fold_device(None, None, None, 0, None, 1),
        lambda: L.gs_spanner_add(None, None, None, 0),
        lambda: L.gs_spanner_within(None, None, None, 0, 3, None),
        lambda: L.gs_spanner_within_device(None, None, None, 0, 3, None),
        lambda: L.gs_spanner_combine(None, None),
        lambda: L.gs_spanner_count(None, ctypes.byref(w), ctypes.byref(w)),
        lambda: L.gs_spanner_export_device(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_spanner_export(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_spanner_neighbors(None, None, None, None, 0, 0, ctypes.byref(n), ctypes.byref(n)),
        lambda: L.gs_spanner_sync(None),
        lambda: L.gs_spanner_get_stream(None, ctypes.byref(p)),
        lambda: L.gs_spanner_wait_stream(None, None),
        lambda: L.gs_testing_spanner_stats(None, ctypes.byref(w)),
        lambda: L.gs_testing_spanner_generation(None, -1, ctypes.byref(w)),
    )
    for c in calls:
        assert c() == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()
    assert L.gs_spanner_destroy(None) == gs.GS_OK


def test_k_outside_the_range_is_rejected_before_any_device_call(gs):
    L = gs.lib()
    h = ctypes.c_void_p()
    for k in (0, -1, 17, 1 << 20):
        assert L.gs_spanner_create(ctypes.byref(h), 0, k, 16) == gs.GS_ERR_INVALID
        assert b"1..16" in L.gs_last_error() and not h.value
    assert gs.SPANNER_MAX_K == 16
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_spanner.cpp")) as f:
        text = f.read()
    # both within entry points check k right after the handle: in the one guard they share
    body = text.split("int within_impl(")[1].split("\n}\n")[0]
    assert body.index("check_handle(s") < body.index("check_k(k)") < body.index("DeviceGuard")
    for fn in ("gs_spanner_within_device", "gs_spanner_within"):
        body = text.split("int %s(" % fn)[1].split("\n}\n")[0]
        assert body.split("{")[1].strip().startswith("return within_impl(s, src, dst, n, k, out, "), fn


def test_python_class_has_the_methods(gs):
    for m in ("close", "reset", "sync", "wait_stream", "fold", "fold_device", "add", "within", "within_device", "combine",
              "count", "edges", "edges_device", "neighbors", "stats", "generation", "__enter__", "__exit__"):
        assert callable(getattr(gs.Spanner, m)), m
    assert isinstance(gs.Spanner.stream, property)


def test_spanner_constants_match_the_kernels(gs):
    csrc = os.path.join(ROOT, "gelly-streaming_amd", "csrc")
    with open(os.path.join(csrc, "gs_spanner_seq.hpp")) as f:
        seq = f.read()
    with open(os.path.join(csrc, "gs_spanner.hpp")) as f:
        hpp = f.read()
    assert gs.SPANNER_MAX_K == int(re.search(r"constexpr int kSpannerMaxK = (\d+);", seq).group(1))
    assert gs.SPANNER_LDS_SET == int(re.search(r"constexpr uint32_t kSpannerLdsSet = (\d+);", seq).group(1))
    assert gs.SPANNER_ARENAS == int(re.search(r"constexpr uint32_t kSpannerArenas = (\d+);", hpp).group(1))
    assert gs.SPANNER_ROUND_CAP == int(re.search(r"constexpr uint32_t kSpannerRoundCap = (\d+);", hpp).group(1))
    assert gs.SPANNER_TILE == int(re.search(r"constexpr uint32_t SPANNER_TILE = (\d+);", hpp).group(1)) == 1024
    assert gs.SPANNER_MAX_GEN == int(re.search(r"constexpr uint32_t kSpMaxGen = (0x[0-9A-Fa-f]+)u;", seq).group(1), 16)


def test_spanner_knobs_roundtrip(gs):
    product = {"spanner_round_cap": gs.SPANNER_ROUND_CAP, "spanner_lds_set": gs.SPANNER_LDS_SET,
               "spanner_arenas": gs.SPANNER_ARENAS}
    for k, v in product.items():
        assert gs.testing_get(k) == v
    with gs.testing(spanner_round_cap=1, spanner_lds_set=4, spanner_arenas=1):
        assert gs.testing_get("spanner_round_cap") == 1 and gs.testing_get("spanner_lds_set") == 4
        assert gs.testing_get("spanner_arenas") == 1
    with gs.testing(spanner_round_cap=0):
        assert gs.testing_get("spanner_round_cap") == 0
    for k, v in product.items():
        assert gs.testing_get(k) == v
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        text = f.read()
    assert re.search(r"GS_TESTING_SPANNER_ROUND_CAP = 10,", text) and re.search(r"GS_TESTING_SPANNER_ARENAS = 12,", text)
    assert re.search(r"GS_TESTING_KNOBS = 13\b", text)
    assert gs.lib().gs_testing_set(13, 1) == gs.GS_ERR_INVALID


def test_fixture_is_data_with_citations():
    with open(os.path.join(ROOT, "tests", "golden", "spanner_pins.json")) as f:
        pins = json.load(f)
    for k in ("bounded_bfs", "add_edge", "default_stream"):
        assert ".java:" in pins[k]["cite"], k
    assert [s["within"] for s in pins["bounded_bfs"]["steps"]] == [False, False, True, False, False, True]
    assert len(pins["default_stream"]["edges"]) == 12 and pins["default_stream"]["k"] == 3
    assert pins["default_stream"]["accepted_arrivals"] == [0, 1, 2, 4, 5, 6, 7, 9, 10]

    def leaves(x):
        if isinstance(x, dict):
            return [y for v in x.values() for y in leaves(v)]
        if isinstance(x, list):
            return [y for v in x for y in leaves(v)]
        return [x]
    assert all(isinstance(x, (int, bool, str)) for x in leaves(pins))
    assert all(".java:" in x for x in leaves(pins) if isinstance(x, str))
