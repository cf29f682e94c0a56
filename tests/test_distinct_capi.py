"""CPU: the distinct streams' entry points exist, are declared in gs_summary.h, exported and bound,
and reject null arguments before touching a device. No compute calls here (the results are
checked on the GPU in test_gpu_distinct.py)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_distinct_create", "gs_distinct_destroy", "gs_distinct_reset", "gs_distinct_fold",
         "gs_distinct_fold_device", "gs_distinct_size", "gs_distinct_new_edges_device", "gs_distinct_new_edges",
         "gs_distinct_new_vertices_device", "gs_distinct_new_vertices", "gs_distinct_vertices_device",
         "gs_distinct_vertices", "gs_distinct_edges_device", "gs_distinct_edges", "gs_distinct_rank_device",
         "gs_distinct_contains_device", "gs_distinct_sync", "gs_distinct_get_stream", "gs_distinct_wait_stream")


def test_names_are_declared_exported_and_bound(gs):
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    L = gs.lib()
    assert re.search(r"typedef struct gs_distinct_s\* gs_distinct;", text)
    assert re.search(r"enum gs_distinct_mode \{ GS_DISTINCT_DIRECTED = 0, GS_DISTINCT_UNDIRECTED = 1 \};", text)
    assert gs.DISTINCT_MODES == {"directed": 0, "undirected": 1}
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert not re.search(r"\d", n)
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
        assert re.search(r"\bint %s\(gs_distinct\*? \w+[,)]" % n, text), n
        assert getattr(L, n).argtypes, n
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    assert "gs_testing_distinct_stats" in gs.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(gs.LIB_PATH), "gs_testing_distinct_stats")
    assert re.search(r"\bint gs_testing_distinct_stats\(void\* d, uint64_t\* out\);", testing)
    assert L.gs_testing_distinct_stats.argtypes
    assert "gs_testing_distinct_phases" in gs.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(gs.LIB_PATH), "gs_testing_distinct_phases")
    assert re.search(r"\bint gs_testing_distinct_phases\(void\* d, uint64_t\* out\);", testing)
    assert L.gs_testing_distinct_phases.argtypes
    assert L.gs_testing_set(99, 1) == gs.GS_ERR_INVALID  # the one knob added is the benchmark's


def test_header_records_the_relation_to_the_reference():
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    section = text[text.index("---- distinct streams"):text.index("typedef struct gs_distinct_s")]
    for word in ("DistinctEdgeMapper", "TestDistinct", "first occurrence", "getVertices", "GS_ERR_CAPACITY"):
        assert word in section, word


def test_null_handles_and_pointers_are_rejected(gs):
    L = gs.lib()
    n = ctypes.c_size_t(7)
    w = ctypes.c_uint64(0)
    p = ctypes.c_void_p()
    wp = ctypes.byref(w)
    calls = (
        lambda: L.gs_distinct_create(None, 0, 0, 16, 16),
        lambda: L.gs_distinct_reset(None),
        lambda: L.gs_distinct_fold(None, None, None, 0),
        lambda: L.gs_distinct_fold_device(None, None, None, 0, 1),
        lambda: L.gs_distinct_size(None, wp, wp, wp, wp, wp),
        lambda: L.gs_distinct_new_edges_device(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_distinct_new_edges(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_distinct_new_vertices_device(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_distinct_new_vertices(None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_distinct_vertices_device(None, None, 0, ctypes.byref(n)),
        lambda: L.gs_distinct_vertices(None, None, 0, ctypes.byref(n)),
        lambda: L.gs_distinct_edges_device(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_distinct_edges(None, None, None, None, 0, ctypes.byref(n)),
        lambda: L.gs_distinct_rank_device(None, None, 0, None, None),
        lambda: L.gs_distinct_contains_device(None, None, None, 0, None),
        lambda: L.gs_distinct_sync(None),
        lambda: L.gs_distinct_get_stream(None, ctypes.byref(p)),
        lambda: L.gs_distinct_wait_stream(None, None),
        lambda: L.gs_testing_distinct_stats(None, wp),
        lambda: L.gs_testing_distinct_phases(None, wp),
    )
    for c in calls:
        assert c() == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()
    assert n.value == 7  # nothing was written
    assert L.gs_distinct_destroy(None) == gs.GS_OK


def test_unknown_mode_is_rejected_before_any_device_call(gs):
    L = gs.lib()
    h = ctypes.c_void_p()
    for mode in (-1, 2, 7):
        assert L.gs_distinct_create(ctypes.byref(h), 0, mode, 0, 0) == gs.GS_ERR_INVALID
        assert b"mode" in L.gs_last_error() and not h.value


def test_distinct_profile_knob_roundtrip(gs):
    assert gs.testing_get("distinct_profile") == 0
    with gs.testing(distinct_profile=1):
        assert gs.testing_get("distinct_profile") == 1
    assert gs.testing_get("distinct_profile") == 0


def test_python_class_has_the_methods(gs):
    for m in ("close", "sync", "wait_stream", "reset", "fold", "fold_device", "size", "new_edges", "new_edges_device",
              "new_vertices", "new_vertices_device", "vertices", "vertices_device", "edges", "edges_device",
              "rank_device", "contains_device", "stats", "phases", "__enter__", "__exit__"):
        assert callable(getattr(gs.Distinct, m)), m
    assert isinstance(gs.Distinct.stream, property) and isinstance(gs.Distinct.handle, property)


def test_distinct_tile_matches_the_kernels(gs):
    """gsamd.DISTINCT_TILE (the size test_gpu_distinct.py brackets) is the kernel header's: threads
    x consecutive positions per thread of the flag and write kernels."""
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_distinct.hpp")) as f:
        text = f.read()
    tile = int(re.search(r"constexpr uint32_t DISTINCT_TILE = (\d+);", text).group(1))
    bs = int(re.search(r"constexpr uint32_t kDistBS = (\d+);", text).group(1))
    assert re.search(r"kDistPer = DISTINCT_TILE / kDistBS;", text) and tile % bs == 0
    assert gs.DISTINCT_TILE == tile and bs == 256


def test_fixture_is_data_with_citations():
    with open(os.path.join(ROOT, "tests", "golden", "distinct_pins.json")) as f:
        pins = json.load(f)
    for k, v in pins.items():
        assert isinstance(v["cite"], str) and ".java:" in v["cite"], k
    assert "GraphStreamTestUtils.java:56-67" in pins["edges"]["cite"] and len(pins["edges"]["rows"]) == 7
    assert "TestDistinct.java:38-51" in pins["distinct"]["cite"] and pins["distinct"]["input_repeats"] == 2
    assert pins["distinct"]["rows"] == pins["edges"]["rows"]
    assert "TestGetVertices.java:38-42" in pins["vertices"]["cite"] and pins["vertices"]["rows"] == [1, 2, 3, 4, 5]
    assert "TestNumberOfEntities.java:40-44" in pins["number_of_vertices"]["cite"]
    assert "TestNumberOfEntities.java:65-71" in pins["number_of_edges"]["cite"]
    assert len(pins["literal_mapper"]["kept_at_parallelism_one"]) == 5
    assert "five of the seven" in pins["literal_mapper"]["note"]
    # the fixture against itself: the literal mapper (one set of targets) and the contract (a set of pairs)
    targets, pairs, literal, contract, seen, entries = set(), set(), [], [], set(), []
    for i, (s, d, v) in enumerate(pins["edges"]["rows"] * pins["distinct"]["input_repeats"]):
        if d not in targets:
            targets.add(d)
            literal.append([s, d, v])
        if (s, d) not in pairs:
            pairs.add((s, d))
            contract.append([s, d, v])
        for e, x in ((2 * i, s), (2 * i + 1, d)):
            if x not in seen:
                seen.add(x)
                entries.append(e)
    assert literal == pins["literal_mapper"]["kept_at_parallelism_one"]
    assert contract == pins["distinct"]["rows"]
    assert entries == pins["vertices"]["entries"]
