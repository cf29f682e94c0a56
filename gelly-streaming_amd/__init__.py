"""gelly-streaming_amd -- MI355X-native summary aggregation for gelly-streaming.

Python binding (ctypes) of the C ABI in include/gs_summary.h / include/gs_gen.h.
The compute path is lib/libgs_summary.so (hand-written HIP for gfx950); there is
no CPU fallback: constructing a Summary without the library or without a GPU
raises.

The directory name is not a Python identifier; import it through the root-level
shim `gsamd` (``import gsamd``), which loads this package as
``gelly_streaming_amd``.
"""
import ctypes
import os

import numpy as np

# Pipelined folds run on up to four lane streams beside the handle stream (and a group
# adds its communication streams). HIP maps streams onto GPU_MAX_HW_QUEUES hardware
# queues (default 4) and streams that share a queue run in submission order; the
# library is arranged for the default (lanes created on first use, a group's lanes
# ordered behind the handle stream only when it has new work: DESIGN.md section 5), so
# the binding does not change the process's setting.

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgs_summary.so")
if os.environ.get("GS_LIB_VARIANT"):  # debug-counter build (Makefile target `debug`: GS_LIB_VARIANT=debug)
    LIB_PATH = os.path.join(_HERE, "lib_" + os.environ["GS_LIB_VARIANT"], "libgs_summary.so")

KIND_CC = 0
KIND_SIGNED = 1
KIND_DEGREE = 2

DEGREE_ALL = 0  # gs_degree_dir (DegreeTypeSeparator, SimpleEdgeStream.java:440-459)
DEGREE_IN = 1
DEGREE_OUT = 2

GS_OK = 0
GS_ERR_INVALID = -1
GS_ERR_HIP = -2
GS_ERR_CAPACITY = -3
GS_ERR_TRUNCATED = -4
GS_ERR_PARSE = -5

SEP_WHITESPACE = 0  # split("\\s") (ConnectedComponentsExample.java:113)
SEP_TAB = 1         # split("\\t") (BipartitenessCheckExample.java:101)

KERNEL_IDS = {"fold": 0, "stage": 1, "export": 2, "init": 3}

# Every symbol include/gs_summary.h and include/gs_gen.h declare.
EXPORTED_SYMBOLS = (
    "gs_last_error", "gs_version", "gs_create", "gs_destroy", "gs_reset", "gs_fold", "gs_fold_device",
    "gs_combine", "gs_sync", "gs_num_vertices", "gs_find", "gs_export_labels", "gs_export_labels_device",
    "gs_bip_status", "gs_export_colouring", "gs_serialize", "gs_deserialize", "gs_set_delta_tracking",
    "gs_take_delta_records", "gs_fold_take_device", "gs_delta_stage", "gs_fold_records_device", "gs_fold_exchange_device",
    "gs_get_stream", "gs_set_pipelining", "gs_set_hot_index", "gs_hot_index_stats", "gs_testing_hot_tune", "gs_testing_hot_keys", "gs_set_profiling", "gs_kernel_stats", "gs_table_capacity", "gs_counters", "gs_debug_counters",
    "gs_gen_rmat", "gs_gen_er", "gs_gen_bip",
    "gs_parse_edges_device", "gs_fold_text", "gs_parse_set_profiling", "gs_parse_profile", "gs_parse_release",
    "gs_group_unique_id", "gs_group_create", "gs_group_fold_device", "gs_group_finish", "gs_group_stats",
    "gs_group_destroy", "gs_group_tree_combine", "gs_combine_exported_device",
    "gs_group_fold_batches_device", "gs_group_set_ramp", "gs_export_labels_part_device",
    "gs_delta_capacity", "gs_find_labels_device", "gs_capacity_stats",
    "gs_set_change_tracking", "gs_take_changes_device", "gs_take_changes",
    "gs_fold_records_counted_device", "gs_reset_config", "gs_wait_event", "gs_wait_stream", "gs_fold_device_after",
    "gs_fold_parity", "gs_set_window_server", "gs_window_server_stats", "gs_set_batch_dedup",
    "gs_digest", "gs_group_comm_ranks", "gs_group_set_phase_timing", "gs_group_phase_stats",
    "gs_group_set_comm_api", "gs_testing_set", "gs_testing_get", "gs_testing_group_forest", "gs_hbm_bytes", "gs_create_bytes",
    "gs_group_create_partitioned", "gs_group_part_fold_device", "gs_group_part_combine",
    "gs_group_part_labels_device", "gs_group_part_status", "gs_group_part_reset", "gs_group_part_stats",
    "gs_group_part_phase_stats",
    "gs_num_components", "gs_export_components_device", "gs_export_components",
    "gs_degree_fold", "gs_degree_fold_device", "gs_degree_find_device", "gs_degree_export_device",
    "gs_degree_export", "gs_degree_distribution_device", "gs_degree_distribution",
    "gs_triangle_create", "gs_triangle_destroy", "gs_triangle_reset", "gs_triangle_fold", "gs_triangle_fold_device",
    "gs_triangle_count", "gs_triangle_count_device", "gs_triangle_find_device", "gs_triangle_export_device",
    "gs_triangle_export", "gs_triangle_sync", "gs_triangle_get_stream", "gs_triangle_wait_stream",
    "gs_testing_triangle_stats", "gs_testing_triangle_bins",
    "gs_triangle_remove", "gs_triangle_remove_device", "gs_triangle_expire", "gs_triangle_set_refresh",
    "gs_testing_triangle_remove_stats", "gs_testing_triangle_remove_phases", "gs_testing_triangle_set_fold",
    "gs_slice_create", "gs_slice_destroy", "gs_slice_window", "gs_slice_window_device", "gs_slice_size",
    "gs_slice_reduce_device", "gs_slice_reduce", "gs_slice_neighborhoods_device", "gs_slice_neighborhoods",
    "gs_slice_sync", "gs_slice_get_stream", "gs_slice_wait_stream", "gs_testing_slice_stats",
    "gs_distinct_create", "gs_distinct_destroy", "gs_distinct_reset", "gs_distinct_fold", "gs_distinct_fold_device",
    "gs_distinct_size", "gs_distinct_new_edges_device", "gs_distinct_new_edges", "gs_distinct_new_vertices_device",
    "gs_distinct_new_vertices", "gs_distinct_vertices_device", "gs_distinct_vertices", "gs_distinct_edges_device",
    "gs_distinct_edges", "gs_distinct_rank_device", "gs_distinct_contains_device", "gs_distinct_sync",
    "gs_distinct_get_stream", "gs_distinct_wait_stream", "gs_testing_distinct_stats",
    "gs_testing_distinct_phases",
    "gs_spanner_create", "gs_spanner_destroy", "gs_spanner_reset", "gs_spanner_fold", "gs_spanner_fold_device",
    "gs_spanner_add", "gs_spanner_within", "gs_spanner_within_device", "gs_spanner_combine", "gs_spanner_count",
    "gs_spanner_export_device", "gs_spanner_export", "gs_spanner_neighbors", "gs_spanner_sync",
    "gs_spanner_get_stream", "gs_spanner_wait_stream", "gs_testing_spanner_stats",
    "gs_testing_spanner_generation",
    "gs_matching_create", "gs_matching_destroy", "gs_matching_reset", "gs_matching_fold", "gs_matching_fold_device",
    "gs_matching_events", "gs_matching_events_device", "gs_matching_count", "gs_matching_export",
    "gs_matching_export_device", "gs_matching_mate_device", "gs_matching_sync", "gs_matching_get_stream",
    "gs_matching_wait_stream", "gs_testing_matching_stats", "gs_testing_matching_tune",
    "gs_trisample_create", "gs_trisample_destroy", "gs_trisample_reset", "gs_trisample_fold", "gs_trisample_fold_device",
    "gs_trisample_rows", "gs_trisample_rows_device", "gs_trisample_estimate", "gs_trisample_states",
    "gs_trisample_states_device", "gs_trisample_sync", "gs_trisample_get_stream", "gs_trisample_wait_stream",
    "gs_testing_trisample_stats", "gs_testing_trisample_tune",
    "gs_degstream_create", "gs_degstream_destroy", "gs_degstream_reset", "gs_degstream_fold", "gs_degstream_fold_device",
    "gs_degstream_rows", "gs_degstream_rows_device", "gs_degstream_records", "gs_degstream_records_device",
    "gs_degstream_size", "gs_degstream_degrees", "gs_degstream_degrees_device", "gs_degstream_distribution",
    "gs_degstream_distribution_device", "gs_degstream_sync", "gs_degstream_get_stream", "gs_degstream_wait_stream",
    "gs_testing_degstream_stats", "gs_testing_degstream_tune",
    "gs_tristream_create", "gs_tristream_destroy", "gs_tristream_reset", "gs_tristream_fold", "gs_tristream_fold_device",
    "gs_tristream_rows", "gs_tristream_rows_device", "gs_tristream_records", "gs_tristream_records_device",
    "gs_tristream_size", "gs_tristream_count", "gs_tristream_counts", "gs_tristream_counts_device", "gs_tristream_sync",
    "gs_tristream_get_stream", "gs_tristream_wait_stream", "gs_testing_tristream_stats", "gs_testing_tristream_tune",
    "gs_parse_records_device", "gs_window_bounds_device", "gs_text_create", "gs_text_destroy", "gs_text_set_window",
    "gs_text_open", "gs_text_next", "gs_text_windows", "gs_text_position", "gs_text_sync", "gs_text_get_stream", "gs_text_wait_stream",
    "gs_testing_text_stats",
)

TEXT_THIRD = {None: 0, "long": 1, "event": 2}  # GS_TEXT_THIRD_* (include/gs_ingest.h)
TEXT_INT32 = 1            # GS_TEXT_INT32: Integer.parseInt endpoints
TEXT_COMMENT_PERCENT = 2  # GS_TEXT_COMMENT_PERCENT: "%" lines give no record
# Lines per workgroup of the comment compaction and records per workgroup of the window bounds
# (csrc/gs_text_seq.hpp kTxtTile); TILE_SCAN_BLOCK of them per step of the tile scan.
TEXT_TILE = 1024

# Pairs per workgroup of the component export's radix-sort kernels (csrc/gs_sort.hpp kSortTile):
# sizes around it are where a tile fills exactly.
SORT_TILE = 2048
# Tile counts per step of the one-workgroup scan between a flag and a write kernel (csrc/gs_sort.hpp
# kSortScanBS, launch_tile_scan; the slices, the distinct streams and the triangle summary compact
# through it): past TILE_SCAN_BLOCK tiles of SLICE_TILE / DISTINCT_TILE / TRIANGLE_TILE elements the
# scan carries a sum from one step into the next.
TILE_SCAN_BLOCK = 1024

# The union-find fold (csrc/gs_device.hpp kFoldBS, kShards; csrc/gs_kernels.hip GS_COMBINE_ROUNDS):
# edges per workgroup of k_fold (one per thread), the shards a launch's workgroups rotate their
# appends through, and the groups of lanes sharing a larger-key root that one wave combines
# before the rest go to the hook loop uncombined.
FOLD_BLOCK = 256
FOLD_SHARDS = 64
FOLD_COMBINE_ROUNDS = 2

# Edges per workgroup of the degree fold (csrc/gs_degree.hpp DEGREE_TILE): the tile whose
# endpoint occurrences are combined on chip; sizes around it are where a tile fills exactly.
DEGREE_TILE = 2048

# The triangle summary's count step (csrc/gs_triangle.hpp): lanes that share one new edge's
# shorter row in the product, edges per workgroup of the per-edge passes, and the number of
# work assignments gsamd.testing(triangle_variant=...) selects (0 is the product).
TRIANGLE_LANES = 8
TRIANGLE_TILE = 1024
TRIANGLE_VARIANTS = 2
# The product's bins by row length (kTriShortRow, kTriWaveRow, kTriLdsRow, kTriSamples): a new
# edge whose shorter row has at most TRIANGLE_SHORT_ROW entries takes a lane group; one whose
# shorter row has more than TRIANGLE_WAVE_ROW and whose longer row has at least
# TRIANGLE_LDS_ROW takes a workgroup with TRIANGLE_SAMPLES samples of the longer row in LDS;
# every other takes a wave.
TRIANGLE_SHORT_ROW = 32
TRIANGLE_WAVE_ROW = 64
TRIANGLE_LDS_ROW = 4096
TRIANGLE_SAMPLES = 1024

# Sorted positions per workgroup of the window slices' heads and reduce kernels
# (csrc/gs_slice.hpp SLICE_TILE; a thread owns SLICE_TILE / 256 consecutive ones): a segment that
# crosses a multiple of it is joined through carry records.
SLICE_TILE = 2048
SLICE_DIRECTIONS = {"out": 0, "in": 1, "all": 2}  # gs_slice_dir
SLICE_OPS = {"sum": 0, "min": 1, "max": 2, "count": 3}  # gs_slice_op

# Positions per workgroup of the distinct streams' flag and write kernels (csrc/gs_distinct.hpp
# DISTINCT_TILE): the kept entries / edges of a fold are compacted tile by tile.
DISTINCT_TILE = 2048
DISTINCT_MODES = {"directed": 0, "undirected": 1}  # gs_distinct_mode

# The k-spanner summary (csrc/gs_spanner_seq.hpp, csrc/gs_spanner.hpp): the range of k, the vertices
# per side a wave's on-chip sets hold before a search takes the heavy path, the arenas of the
# heavy path's pool and the rounds before the serial tail; the elements per workgroup of the three
# flag / compact passes (SPANNER_TILE) and the generations a stamp arena takes before it is cleared
# (kSpMaxGen).
SPANNER_MAX_K = 16
SPANNER_LDS_SET = 256
SPANNER_TILE = 1024
SPANNER_MAX_GEN = 0x7FFFFFF0
SPANNER_ARENAS = 32
SPANNER_ROUND_CAP = 16

# The weighted matching summary (csrc/gs_matching_seq.hpp, csrc/gs_matching.hpp): the rounds of a
# fold before the one-workgroup tail takes what is left, the pending count below which it takes
# them at once, the fixpoint passes of a round before it falls back to plain reservations, the
# bits of a weight-safe value, and the arrivals per workgroup of the event compaction.
MATCHING_ROUND_CAP = 32
MATCHING_TAIL_THRESHOLD = 4096
MATCHING_ITER_CAP = 6
MATCHING_SAFE_BITS = 61
MATCHING_TILE = 1024
MATCHING_EVENTS = {"add": 0, "remove": 1}  # gs_matching_event

# The sampling triangle estimate (csrc/gs_trisample_seq.hpp): arrivals per workgroup of the coin
# pass and of the search pass, the limits of a handle, the reference's master seed (the Java int
# literal 0xDEADBEEF, widened) and the arrivals of one device fold (longer ones are cut).
TRISAMPLE_CHUNK = 256
TRISAMPLE_TILE = 1024
TRISAMPLE_MAX_SAMPLES = 1 << 20
TRISAMPLE_MAX_VERTICES = (1 << 31) - 1
TRISAMPLE_MAX_ARRIVALS = (1 << 31) - 1
TRISAMPLE_SEED = -559038737
TRISAMPLE_MAX_FOLD = 1 << 20

# The degree streams (csrc/gs_degstream.hpp, csrc/gs_degstream_seq.hpp): sorted positions per
# workgroup of the two seeded segmented scans and of the record compaction (a segment that crosses
# a multiple of it is joined through the scan of the tile aggregates), the count array's first
# capacity in degrees, the occurrences a handle takes between resets and the edges of the largest
# fold whose rows are kept.
DEGSTREAM_TILE = 2048
DEGSTREAM_MIN_COUNTS = 1024
DEGSTREAM_MAX_TOTAL = (1 << 31) - 1
DEGSTREAM_MAX_FOLD = 1 << 24

# The triangle streams (csrc/gs_tristream.hpp, csrc/gs_tristream_seq.hpp): positions per workgroup
# of the scan over the arrivals and of the seeded segmented sum over the records (a segment that
# crosses a multiple of it is joined through the scan of the tile aggregates), the arrivals a
# handle takes between resets, the arrivals of the largest fold whose rows are kept, the records
# one fold may emit, and how a repeated pair is treated (gs_tristream_repeats); the lanes that share
# one arrival's walked row in the intersection while that row has at most TRISTREAM_SHORT_ROW
# entries (a longer one takes a wave of 64).
TRISTREAM_TILE = 2048
TRISTREAM_LANES = 8
TRISTREAM_SHORT_ROW = 32
TRISTREAM_MAX_TOTAL = (1 << 31) - 1
TRISTREAM_MAX_FOLD = 1 << 22
TRISTREAM_MAX_RECORDS = 1 << 27
TRISTREAM_REPEATS = {"count": 0, "ignore": 1}

FAIL_BIT = 1 << 62  # count words: a failed signed verdict (GS_FAIL_BIT)
DIGEST_FAILED = (1 << 64) - 1  # gs_digest of a signed summary whose verdict failed (GS_DIGEST_FAILED)


class GSError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gs error %d: %s" % (code, msg))
        self.code = code


_lib = None
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_u64 = ctypes.c_uint64
_i64 = ctypes.c_int64


def build():
    import subprocess
    subprocess.check_call(["make", "-s", "-C", _HERE, "-j4"])


def lib():
    """Load the HIP library (raises if it was not built: no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libgs_summary.so not built (%s); run __graft_entry__.build()" % LIB_PATH)
    # torch (ROCm 7.0 wheel) bundles its own libamdhip64.so.7 with the same SONAME as
    # /opt/rocm's: whichever loads first serves the whole process. Load torch's first
    # so torch tensors and this library share one HIP runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    L.gs_last_error.restype = ctypes.c_char_p
    L.gs_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, _u64]
    L.gs_destroy.argtypes = [_vp]
    L.gs_reset.argtypes = [_vp]
    L.gs_reset_config.argtypes = [_vp]
    L.gs_fold.argtypes = [_vp, _vp, _vp, _sz]
    L.gs_fold_parity.argtypes = [_vp, _vp, _vp, _vp, _sz]
    L.gs_set_window_server.argtypes = [_vp, ctypes.c_int]
    L.gs_set_batch_dedup.argtypes = [_vp, ctypes.c_int]
    L.gs_window_server_stats.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]
    L.gs_fold_device.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz]
    L.gs_fold_device_after.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, _vp]
    L.gs_wait_event.argtypes = [_vp, _vp]
    L.gs_wait_stream.argtypes = [_vp, _vp]
    L.gs_combine.argtypes = [_vp, _vp]
    L.gs_sync.argtypes = [_vp]
    L.gs_num_vertices.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_find.argtypes = [_vp, _i64, ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_int)]
    L.gs_export_labels.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_export_labels_device.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_bip_status.argtypes = [_vp, ctypes.POINTER(ctypes.c_int)]
    L.gs_export_colouring.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_serialize.argtypes = [_vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_deserialize.argtypes = [_vp, _vp, _sz]
    L.gs_set_delta_tracking.argtypes = [_vp, ctypes.c_int]
    L.gs_take_delta_records.argtypes = [_vp, _vp, _sz, _vp]
    L.gs_fold_take_device.argtypes = [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]
    L.gs_fold_records_device.argtypes = [_vp, _vp, _sz, ctypes.c_int]
    L.gs_fold_records_counted_device.argtypes = [_vp, _vp, _sz, _vp, ctypes.c_int]
    L.gs_delta_stage.argtypes = [_vp, _vp, _sz, ctypes.c_int, _vp]
    L.gs_fold_exchange_device.argtypes = [_vp, _vp, _vp, _sz, _sz, ctypes.c_int, ctypes.c_int]
    L.gs_delta_capacity.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_find_labels_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.gs_capacity_stats.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double)]
    L.gs_set_change_tracking.argtypes = [_vp, ctypes.c_int]
    L.gs_take_changes_device.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_u64)]
    L.gs_take_changes.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_u64)]
    L.gs_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_set_profiling.argtypes = [_vp, ctypes.c_int]
    L.gs_set_pipelining.argtypes = [_vp, ctypes.c_int]
    L.gs_set_hot_index.argtypes = [_vp, ctypes.c_int, _u64, ctypes.c_uint32]
    L.gs_hot_index_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    if hasattr(L, "gs_testing_hot_tune"):  # (an A/B's GS_LIB_VARIANT library of the parent commit has neither)
        L.gs_testing_hot_tune.argtypes = [_vp, ctypes.c_int, ctypes.c_int64]
        L.gs_testing_hot_keys.argtypes = [_vp, ctypes.POINTER(_i64), _u64]
        L.gs_testing_hot_keys.restype = _i64
    L.gs_kernel_stats.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double)]
    L.gs_table_capacity.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_counters.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_debug_counters.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.c_int]
    L.gs_gen_rmat.argtypes = [_vp, _vp, _vp, _u64, _u64, ctypes.c_int, _u64, ctypes.c_int]
    L.gs_gen_er.argtypes = [_vp, _vp, _vp, _u64, _u64, ctypes.c_int, _u64, ctypes.c_int]
    L.gs_gen_bip.argtypes = [_vp, _vp, _vp, _u64, _u64, ctypes.c_int, _u64, _vp, _sz]
    L.gs_parse_edges_device.argtypes = [_vp, _vp, _sz, ctypes.c_int, _vp, _vp, _sz, ctypes.POINTER(_u64),
                                        ctypes.POINTER(_i64)]
    L.gs_parse_set_profiling.argtypes = [ctypes.c_int]
    L.gs_parse_profile.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_u64)]
    L.gs_fold_text.argtypes = [_vp, ctypes.c_char_p, _sz, ctypes.c_int, ctypes.POINTER(_u64), ctypes.POINTER(_i64)]
    if hasattr(L, "gs_text_create"):  # (an A/B's GS_LIB_VARIANT library of the parent commit has none of them)
        L.gs_parse_records_device.argtypes = [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
                                              _vp, _sz, ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                                              ctypes.POINTER(_i64)]
        L.gs_window_bounds_device.argtypes = [_vp, _vp, _sz, _i64, _vp, _vp, _sz, ctypes.POINTER(_u64)]
        L.gs_text_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _sz]
        L.gs_text_destroy.argtypes = [_vp]
        L.gs_text_set_window.argtypes = [_vp, _i64]
        L.gs_text_open.argtypes = [_vp, _vp, _sz]
        L.gs_text_next.argtypes = [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                   ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                   ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_int)]
        L.gs_text_windows.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
        L.gs_text_position.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_i64)]
        L.gs_text_sync.argtypes = [_vp]
        L.gs_text_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
        L.gs_text_wait_stream.argtypes = [_vp, _vp]
        L.gs_testing_text_stats.argtypes = [ctypes.POINTER(_u64)]
    L.gs_group_unique_id.argtypes = [_vp]
    L.gs_group_create.argtypes = [ctypes.POINTER(_vp), _vp, _vp, ctypes.c_int, ctypes.c_int, _sz]
    L.gs_group_fold_device.argtypes = [_vp, _vp, _vp, _sz]
    L.gs_group_finish.argtypes = [_vp]
    L.gs_group_stats.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64)]
    L.gs_group_destroy.argtypes = [_vp]
    L.gs_group_tree_combine.argtypes = [_vp]
    L.gs_group_fold_batches_device.argtypes = [_vp, _vp, _vp, _sz, _sz]
    L.gs_group_set_ramp.argtypes = [_vp, _sz, _sz]
    L.gs_export_labels_part_device.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _sz,
                                               ctypes.POINTER(_sz)]
    L.gs_combine_exported_device.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.c_int]
    L.gs_digest.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_group_comm_ranks.argtypes = [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.gs_group_set_phase_timing.argtypes = [_vp, ctypes.c_int]
    L.gs_group_phase_stats.argtypes = [_vp, ctypes.POINTER(ctypes.c_double)]
    L.gs_group_set_comm_api.argtypes = [_vp]
    L.gs_group_create_partitioned.argtypes = [ctypes.POINTER(_vp), _vp, _vp, ctypes.c_int, ctypes.c_int, _u64, _sz]
    L.gs_group_part_fold_device.argtypes = [_vp, _vp, _vp, _sz]
    L.gs_group_part_combine.argtypes = [_vp]
    L.gs_group_part_labels_device.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_group_part_status.argtypes = [_vp, ctypes.POINTER(ctypes.c_int)]
    L.gs_group_part_reset.argtypes = [_vp]
    L.gs_group_part_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_group_part_phase_stats.argtypes = [_vp, ctypes.POINTER(ctypes.c_double)]
    L.gs_hbm_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(_u64)]
    L.gs_create_bytes.argtypes = [ctypes.c_int, _u64, ctypes.POINTER(_u64)]
    L.gs_num_components.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_export_components_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _sz, ctypes.POINTER(_sz),
                                              ctypes.POINTER(_sz)]
    L.gs_export_components.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _sz, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    L.gs_degree_fold.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.c_int]
    L.gs_degree_fold_device.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, ctypes.c_int]
    L.gs_degree_find_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.gs_degree_export_device.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz), ctypes.c_int]
    L.gs_degree_export.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz), ctypes.c_int]
    L.gs_degree_distribution_device.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_degree_distribution.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_triangle_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, _u64]
    L.gs_triangle_destroy.argtypes = [_vp]
    L.gs_triangle_reset.argtypes = [_vp]
    L.gs_triangle_fold.argtypes = [_vp, _vp, _vp, _sz]
    L.gs_triangle_fold_device.argtypes = [_vp, _vp, _vp, _sz, _sz]
    L.gs_triangle_count.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64)]
    L.gs_triangle_count_device.argtypes = [_vp, _vp]
    L.gs_triangle_find_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.gs_triangle_export_device.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz), ctypes.c_int]
    L.gs_triangle_export.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz), ctypes.c_int]
    L.gs_triangle_sync.argtypes = [_vp]
    L.gs_triangle_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_triangle_wait_stream.argtypes = [_vp, _vp]
    L.gs_testing_triangle_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_triangle_bins.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_triangle_remove.argtypes = [_vp, _vp, _vp, _sz]
    L.gs_triangle_remove_device.argtypes = [_vp, _vp, _vp, _sz, _sz]
    L.gs_triangle_expire.argtypes = [_vp, _u64]
    L.gs_triangle_set_refresh.argtypes = [_vp, ctypes.c_int]
    L.gs_testing_triangle_remove_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_triangle_remove_phases.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_triangle_set_fold.argtypes = [_vp, _u64]
    L.gs_slice_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, _u64]
    L.gs_slice_destroy.argtypes = [_vp]
    L.gs_slice_window.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.c_int]
    L.gs_slice_window_device.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, ctypes.c_int]
    L.gs_slice_size.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]
    L.gs_slice_reduce_device.argtypes = [_vp, ctypes.c_int, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_slice_reduce.argtypes = [_vp, ctypes.c_int, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_slice_neighborhoods_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _sz, ctypes.POINTER(_sz),
                                                ctypes.POINTER(_sz)]
    L.gs_slice_neighborhoods.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _sz, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    L.gs_slice_sync.argtypes = [_vp]
    L.gs_slice_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_slice_wait_stream.argtypes = [_vp, _vp]
    L.gs_testing_slice_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_distinct_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, _u64, _u64]
    L.gs_distinct_destroy.argtypes = [_vp]
    L.gs_distinct_reset.argtypes = [_vp]
    L.gs_distinct_fold.argtypes = [_vp, _vp, _vp, _sz]
    L.gs_distinct_fold_device.argtypes = [_vp, _vp, _vp, _sz, _sz]
    L.gs_distinct_size.argtypes = [_vp] + [ctypes.POINTER(_u64)] * 5
    L.gs_distinct_new_edges_device.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_distinct_new_edges.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_distinct_new_vertices_device.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_distinct_new_vertices.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_distinct_vertices_device.argtypes = [_vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_distinct_vertices.argtypes = [_vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_distinct_edges_device.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_distinct_edges.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_distinct_rank_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.gs_distinct_contains_device.argtypes = [_vp, _vp, _vp, _sz, _vp]
    L.gs_distinct_sync.argtypes = [_vp]
    L.gs_distinct_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_distinct_wait_stream.argtypes = [_vp, _vp]
    L.gs_testing_distinct_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_distinct_phases.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_spanner_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, _u64]
    L.gs_spanner_destroy.argtypes = [_vp]
    L.gs_spanner_reset.argtypes = [_vp]
    L.gs_spanner_fold.argtypes = [_vp, _vp, _vp, _sz, _vp]
    L.gs_spanner_fold_device.argtypes = [_vp, _vp, _vp, _sz, _vp, _sz]
    L.gs_spanner_add.argtypes = [_vp, _vp, _vp, _sz]
    L.gs_spanner_within.argtypes = [_vp, _vp, _vp, _sz, ctypes.c_int, _vp]
    L.gs_spanner_within_device.argtypes = [_vp, _vp, _vp, _sz, ctypes.c_int, _vp]
    L.gs_spanner_combine.argtypes = [_vp, _vp]
    L.gs_spanner_count.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]
    L.gs_spanner_export_device.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_spanner_export.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_spanner_neighbors.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    L.gs_spanner_sync.argtypes = [_vp]
    L.gs_spanner_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_spanner_wait_stream.argtypes = [_vp, _vp]
    L.gs_testing_spanner_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_spanner_generation.argtypes = [_vp, ctypes.c_int64, ctypes.POINTER(_u64)]
    L.gs_matching_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, _u64]
    L.gs_matching_destroy.argtypes = [_vp]
    L.gs_matching_reset.argtypes = [_vp]
    L.gs_matching_fold.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp]
    L.gs_matching_fold_device.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _sz]
    L.gs_matching_events.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_matching_events_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_matching_count.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_int64)]
    L.gs_matching_export.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_matching_export_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_matching_mate_device.argtypes = [_vp, _vp, _sz, _vp, _vp, _vp]
    L.gs_matching_sync.argtypes = [_vp]
    L.gs_matching_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_matching_wait_stream.argtypes = [_vp, _vp]
    L.gs_testing_matching_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_matching_tune.argtypes = [_vp, ctypes.c_int, ctypes.c_int64]
    L.gs_trisample_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, _u64, ctypes.c_int64, ctypes.c_int64, _u64]
    L.gs_trisample_destroy.argtypes = [_vp]
    L.gs_trisample_reset.argtypes = [_vp]
    L.gs_trisample_fold.argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_trisample_fold_device.argtypes = [_vp, _vp, _vp, _sz, _sz, ctypes.POINTER(_sz)]
    L.gs_trisample_rows.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_trisample_rows_device.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_trisample_estimate.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(ctypes.c_int32)]
    L.gs_trisample_states.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
    L.gs_trisample_states_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
    L.gs_trisample_sync.argtypes = [_vp]
    L.gs_trisample_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_trisample_wait_stream.argtypes = [_vp, _vp]
    L.gs_testing_trisample_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_trisample_tune.argtypes = [_vp, ctypes.c_int, ctypes.c_int64]
    L.gs_degstream_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, _u64]
    L.gs_degstream_destroy.argtypes = [_vp]
    L.gs_degstream_reset.argtypes = [_vp]
    L.gs_degstream_fold.argtypes = [_vp, _vp, _vp, _vp, _sz]
    L.gs_degstream_fold_device.argtypes = [_vp, _vp, _vp, _vp, _sz, _sz]
    for name in ("rows", "records"):
        getattr(L, "gs_degstream_" + name).argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
        getattr(L, "gs_degstream_" + name + "_device").argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    for name in ("degrees", "distribution"):
        getattr(L, "gs_degstream_" + name).argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
        getattr(L, "gs_degstream_" + name + "_device").argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_degstream_size.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_degstream_sync.argtypes = [_vp]
    L.gs_degstream_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_degstream_wait_stream.argtypes = [_vp, _vp]
    L.gs_testing_degstream_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_degstream_tune.argtypes = [_vp, ctypes.c_int, ctypes.c_int64]
    L.gs_tristream_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, _u64]
    L.gs_tristream_destroy.argtypes = [_vp]
    L.gs_tristream_reset.argtypes = [_vp]
    L.gs_tristream_fold.argtypes = [_vp, _vp, _vp, _sz]
    L.gs_tristream_fold_device.argtypes = [_vp, _vp, _vp, _sz, _sz]
    for name in ("rows", "counts"):
        getattr(L, "gs_tristream_" + name).argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
        getattr(L, "gs_tristream_" + name + "_device").argtypes = [_vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_tristream_records.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_tristream_records_device.argtypes = [_vp, _vp, _vp, _vp, _sz, ctypes.POINTER(_sz)]
    L.gs_tristream_size.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_tristream_count.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_tristream_sync.argtypes = [_vp]
    L.gs_tristream_get_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.gs_tristream_wait_stream.argtypes = [_vp, _vp]
    L.gs_testing_tristream_stats.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.gs_testing_tristream_tune.argtypes = [_vp, ctypes.c_int, ctypes.c_int64]
    L.gs_testing_set.argtypes = [ctypes.c_int, _i64]
    L.gs_testing_get.argtypes = [ctypes.c_int]
    L.gs_testing_get.restype = _i64
    L.gs_testing_group_forest.argtypes = [_vp, ctypes.POINTER(_vp)]
    _lib = L
    return L


def hbm_bytes(device=0):
    """gs_hbm_bytes: device memory held by every live summary / group of this process."""
    b = _u64()
    _check(lib().gs_hbm_bytes(int(device), ctypes.byref(b)))
    return b.value


def create_bytes(kind, capacity_hint):
    """gs_create_bytes: the device bytes gs_create(kind, capacity_hint) allocates."""
    b = _u64()
    k = {"cc": KIND_CC, "signed": KIND_SIGNED, "degree": KIND_DEGREE}[kind] if isinstance(kind, str) else int(kind)
    _check(lib().gs_create_bytes(k, int(capacity_hint), ctypes.byref(b)))
    return b.value


def digest_rows(v, label, parity=None):
    """gs_digest's order-independent terms (csrc/gs_kernels.hip digest_term) summed over rows
    of device tensors, mod 2^64: the owned slices of a partitioned group sum to the digest of
    the single summary of the same stream."""
    import torch

    def srl(x, k):  # logical shift right on int64 tensors
        return (x >> k) & ((1 << (64 - k)) - 1)

    def mix(z):
        z = (z ^ srl(z, 30)) * -4658895280553007687  # 0xBF58476D1CE4E5B9 as int64
        z = (z ^ srl(z, 27)) * -7723592293110705685  # 0x94D049BB133111EB
        return z ^ srl(z, 31)
    if v.numel() == 0:
        return 0
    a = mix(v ^ 0x243F6A8885A308D3)
    b = mix(label + (parity.to(torch.int64) * 0x13198A2E03707344 if parity is not None else 0))
    return int(torch.sum(a * b).item()) & ((1 << 64) - 1)


# ---------------------------------------------------------------- test controls
# include/gs_testing.h: private knobs the tests use (the product reads no environment)
TESTING_KNOBS = {"server_idle_us": 0, "changes_walk_max": 1, "parse_lb_timeout_us": 2, "group_self_apply": 3,
                 "group_data_lag": 4, "degree_variant": 5, "triangle_variant": 6, "triangle_profile": 7,
                 "slice_profile": 8, "distinct_profile": 9, "spanner_round_cap": 10, "spanner_lds_set": 11,
                 "spanner_arenas": 12}


def testing_set(knob, value):
    """gs_testing_set: a test knob (name of TESTING_KNOBS) to `value`; None or < 0
    restores the product value."""
    _check(lib().gs_testing_set(TESTING_KNOBS[knob], -1 if value is None else int(value)))


def testing_get(knob):
    return lib().gs_testing_get(TESTING_KNOBS[knob])


def testing_hot_tune(summary, rows=None, sketch_log2=None, sample_folds=None):
    """gs_testing_hot_tune, per handle of a "cc" Summary: the rows of the hot index build's
    sketch (1 or 2), its counters per row and id (log2), the folds counted for one build (1, 2
    or 4). A value < 0 restores the library's. Drops a live index."""
    for what, v in enumerate((rows, sketch_log2, sample_folds)):
        if v is not None:
            _check(lib().gs_testing_hot_tune(summary._h, what, int(v)))


def testing_hot_keys(summary):
    """gs_testing_hot_keys: the keys the live hot index of a "cc" Summary holds (an int64 array,
    in bucket order)."""
    import numpy as np
    n = lib().gs_testing_hot_keys(summary._h, None, 0)
    if n < 0:
        _check(int(n))
    out = (_i64 * max(int(n), 1))()
    m = lib().gs_testing_hot_keys(summary._h, out, int(n))
    if m < 0:
        _check(int(m))
    return np.frombuffer(out, dtype=np.int64, count=int(min(n, m))).copy()


class testing:
    """Context manager: `with gsamd.testing(server_idle_us=100): ...` sets test knobs
    and restores the product values on exit."""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            testing_set(k, v)
        return self

    def __exit__(self, *a):
        for k in self.knobs:
            testing_set(k, None)


FAKE_COMM_PATH = os.path.join(_HERE, "host", "bin", "libgs_fakecomm.so")
_fake = None


def fake_comm():
    """The in-process collectives emulation (tests/cpp/gs_fake_comm.cpp; test
    infrastructure, built by the host Makefile)."""
    global _fake
    if _fake is None:
        lib()  # (torch's HIP runtime first)
        if not os.path.exists(FAKE_COMM_PATH):
            raise ImportError("libgs_fakecomm.so not built (%s); run __graft_entry__.build()" % FAKE_COMM_PATH)
        F = ctypes.CDLL(FAKE_COMM_PATH)
        F.gs_fake_comm_api.restype = _vp
        F.gs_fake_comm_last_error.restype = ctypes.c_int
        F.gs_fake_comm_order_hash.restype = _u64
        _fake = F
    return _fake


def use_comm_emulation(on=True):
    """gs_group_set_comm_api: groups created afterwards run their collectives through the
    in-process emulation (N rank threads on one GPU; it fails a collective whose ranks
    issued the communicators' collectives in different orders) -- or RCCL again (False)."""
    _check(lib().gs_group_set_comm_api(fake_comm().gs_fake_comm_api() if on else None))


class comm_emulation:
    """Context manager around use_comm_emulation(True)."""

    def __enter__(self):
        use_comm_emulation(True)
        return self

    def __exit__(self, *a):
        use_comm_emulation(False)


def _check(rc):
    if rc != GS_OK:
        raise GSError(rc, lib().gs_last_error().decode())
    return rc


def _ptr(x):
    """Device/host address of a torch tensor, numpy array, int or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data
    raise TypeError(type(x))


def _int64s(x):
    """x as a contiguous int64 numpy array (what the host entry points read)."""
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


def _edges(src, dst):
    """The two endpoint arrays of a host fold, of one shape."""
    s, d = _int64s(src), _int64s(dst)
    assert s.shape == d.shape
    return s, d


class _Handle:
    """The owner of one C handle, and the entry points every handle type has. A subclass names
    its C prefix (_PREFIX = "gs_triangle": gs_triangle_destroy, gs_triangle_sync,
    gs_triangle_get_stream, gs_triangle_wait_stream), creates the handle into self._h and sets
    self.device."""

    _PREFIX = None

    def _call(self, name, *args):
        _check(getattr(lib(), "%s_%s" % (self._PREFIX, name))(self._h, *args))

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._PREFIX + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        """The handle's stream (a raw hipStream_t): device entry points queue their work there."""
        s = _vp()
        self._call("get_stream", ctypes.byref(s))
        return s.value

    def sync(self):
        self._call("sync")

    def wait_stream(self, stream="torch"):
        """Every later operation of the handle waits (on the device) for the work queued on
        `stream` so far: a torch.cuda.Stream, a raw hipStream_t, or "torch" (torch's current
        stream). <prefix>_wait_stream."""
        if isinstance(stream, str):
            import torch
            stream = torch.cuda.current_stream(self.device)
        self._call("wait_stream", stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))


class _ResetHandle(_Handle):
    """A handle type with <prefix>_reset."""

    def reset(self):
        """Back to the empty state; capacity is kept (and what the class's docstring names)."""
        self._call("reset")


class Summary(_ResetHandle):
    """One GPU-resident summary (DisjointSet for kind 'cc', signed forest for
    kind 'signed'). Thin owner of a gs_handle; see include/gs_summary.h."""

    _PREFIX = "gs"

    def __init__(self, kind="cc", device=0, capacity_hint=1 << 20):
        self.kind = {"cc": KIND_CC, "signed": KIND_SIGNED}[kind] if isinstance(kind, str) else int(kind)
        self.device = device
        h = _vp()
        _check(lib().gs_create(ctypes.byref(h), device, self.kind, capacity_hint))
        self._h = h
        # A/B runs: GS_HOT_INDEX=0 turns the hot index's default off (set_hot_index still forces it)
        if self.kind == KIND_CC and os.environ.get("GS_HOT_INDEX") == "0":
            _check(lib().gs_set_hot_index(h, -1, 0, 0))

    def reset_config(self):
        """gs_reset_config: reset plus the default configuration (tracking off,
        pipelining 1, profiling off), as a handle pool's release does."""
        _check(lib().gs_reset_config(self._h))

    # --- fold / combine
    def fold(self, src, dst):
        """Fold host edges (int64 numpy arrays or sequences)."""
        s, d = _edges(src, dst)
        _check(lib().gs_fold(self._h, s.ctypes.data, d.ctypes.data, len(s)))

    def fold_parity(self, src, dst, w):
        """Fold host edges with a required parity each (gs_fold_parity; signed kind:
        w = 1 different sides, 0 same side)."""
        s, d = _edges(src, dst)
        ww = np.ascontiguousarray(np.asarray(w, dtype=np.uint8))
        assert s.shape == ww.shape
        _check(lib().gs_fold_parity(self._h, s.ctypes.data, d.ctypes.data, ww.ctypes.data, len(s)))

    def fold_device(self, src, dst, n=None, stride=1, w=None, after=None):
        """Fold device-resident edges (torch tensors on this device or raw pointers).
        The fold is queued on the summary's stream (`self.stream`), not torch's: edges
        written on another stream must be complete first -- pass that stream as
        `after` (a torch.cuda.Stream, or "torch" for torch's current stream; the
        summary's work then waits for it on the device, gs_wait_stream), or
        synchronise, as for any caller of gs_fold_device."""
        if n is None:
            n = src.numel() // (stride if stride > 1 else 1) if hasattr(src, "numel") else None
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_fold_device(self._h, _ptr(src), _ptr(dst), _ptr(w), int(n), int(stride)))

    def wait_event(self, event):
        """Every later operation waits for a recorded torch.cuda.Event (or raw hipEvent_t)."""
        raw = event.cuda_event if hasattr(event, "cuda_event") else int(event)
        _check(lib().gs_wait_event(self._h, raw))

    def combine(self, other):
        _check(lib().gs_combine(self._h, other._h))

    # --- queries
    def num_vertices(self):
        n = _u64()
        _check(lib().gs_num_vertices(self._h, ctypes.byref(n)))
        return n.value

    def find(self, v):
        lab = _i64()
        found = ctypes.c_int()
        _check(lib().gs_find(self._h, int(v), ctypes.byref(lab), ctypes.byref(found)))
        return lab.value if found.value else None

    def find_labels_device(self, v, label, found=None, n=None):
        """Batched find (gs_find_labels_device): label[i] = canonical label of the
        DEVICE id v[i]; found[i] = 0 for an id never seen. Asynchronous on self.stream."""
        n = v.numel() if n is None else n
        _check(lib().gs_find_labels_device(self._h, _ptr(v), int(n), _ptr(label), _ptr(found)))

    def labels(self):
        """(vertex, canonical label) numpy arrays, sorted by vertex."""
        n = self.num_vertices()
        v = np.empty(n, np.int64)
        lab = np.empty(n, np.int64)
        got = _sz()
        _check(lib().gs_export_labels(self._h, v.ctypes.data, lab.ctypes.data, n, ctypes.byref(got)))
        o = np.argsort(v[: got.value], kind="stable")
        return v[: got.value][o], lab[: got.value][o]

    def export_labels_part_device(self, part, nparts, v, label, parity=None):
        """Part `part` of `nparts` disjoint slot ranges of export_labels_device."""
        got = _sz()
        cap = v.numel() if hasattr(v, "numel") else len(v)
        _check(lib().gs_export_labels_part_device(self._h, int(part), int(nparts), _ptr(v), _ptr(label),
                                                  _ptr(parity), cap, ctypes.byref(got)))
        return got.value

    def combine_exported_device(self, v, label, parity, n, failed=False):
        """Fold another summary's exported (v, label, parity) DEVICE arrays into this
        one and AND the verdict with `not failed` (gs_combine_exported_device)."""
        _check(lib().gs_combine_exported_device(self._h, _ptr(v), _ptr(label), _ptr(parity), int(n),
                                                int(bool(failed))))

    def export_labels_device(self, v, label, parity=None):
        got = _sz()
        cap = v.numel() if hasattr(v, "numel") else len(v)
        _check(lib().gs_export_labels_device(self._h, _ptr(v), _ptr(label), _ptr(parity), cap, ctypes.byref(got)))
        return got.value

    def digest(self):
        """gs_digest: order-independent 64-bit digest of the (vertex, label, parity) set
        (DIGEST_FAILED for a failed signed summary). Synchronises."""
        d = _u64()
        _check(lib().gs_digest(self._h, ctypes.byref(d)))
        return d.value

    def ok(self):
        o = ctypes.c_int()
        _check(lib().gs_bip_status(self._h, ctypes.byref(o)))
        return bool(o.value)

    def colouring(self):
        """(ok, comp, v, sign) sorted by (comp, v); empty arrays when not bipartite."""
        n = self.num_vertices()
        comp = np.empty(max(n, 1), np.int64)
        v = np.empty(max(n, 1), np.int64)
        sign = np.empty(max(n, 1), np.uint8)
        got = _sz()
        _check(lib().gs_export_colouring(self._h, comp.ctypes.data, v.ctypes.data, sign.ctypes.data, max(n, 1),
                                         ctypes.byref(got)))
        k = got.value
        comp, v, sign = comp[:k], v[:k], sign[:k]
        o = np.lexsort((v, comp))
        return self.ok(), comp[o], v[o], sign[o]

    def num_components(self):
        """gs_num_components: the number of components (0 for a failed signed summary)."""
        n = _u64()
        _check(lib().gs_num_components(self._h, ctypes.byref(n)))
        return n.value

    def components_device(self, comp, offset, member, sign=None):
        """gs_export_components_device: the summary grouped and ordered as CSR into DEVICE
        arrays (comp int64[cap_c], offset uint64/int64[cap_c + 1], member int64[cap_v], sign
        uint8[cap_v] or None); returns (nv, nc). Raises GSError(GS_ERR_TRUNCATED) when a
        capacity is too small (nothing written)."""
        nv, nc = _sz(), _sz()
        cap_v = member.numel() if hasattr(member, "numel") else len(member)
        cap_c = comp.numel() if hasattr(comp, "numel") else len(comp)
        n_off = offset.numel() if hasattr(offset, "numel") else len(offset)
        assert n_off >= cap_c + 1, "offset holds one entry more than comp"
        _check(lib().gs_export_components_device(self._h, _ptr(comp), _ptr(offset), _ptr(member), _ptr(sign),
                                                 cap_v, cap_c, ctypes.byref(nv), ctypes.byref(nc)))
        return nv.value, nc.value

    def components(self):
        """(ok, comp, offset, member, sign) numpy arrays through gs_export_components: comp
        ascending, offset[nc + 1] into member, member ordered by (label, vertex), sign = 1
        for the colour of the component's minimum (all 0 for kind 'cc'). A failed signed
        verdict gives ok False and empty arrays with offset == [0]."""
        nv, nc = _sz(), _sz()
        n = self.num_vertices()
        k = n  # at most one component per vertex: no count pass before the export
        while True:
            comp = np.empty(k, np.int64)
            offset = np.zeros(k + 1, np.uint64)
            member = np.empty(n, np.int64)
            sign = np.empty(n, np.uint8)
            rc = lib().gs_export_components(self._h, comp.ctypes.data, offset.ctypes.data, member.ctypes.data,
                                            sign.ctypes.data, n, k, ctypes.byref(nv), ctypes.byref(nc))
            if rc != GS_ERR_TRUNCATED:
                break
            n, k = nv.value, nc.value  # (the summary grew between the count and the export)
        _check(rc)
        ok = self.ok() if self.kind == KIND_SIGNED else True
        return ok, comp[: nc.value], offset[: nc.value + 1], member[: nv.value], sign[: nv.value]

    def serialize(self):
        ln = _sz()
        _check(lib().gs_serialize(self._h, None, 0, ctypes.byref(ln)))
        buf = ctypes.create_string_buffer(ln.value)
        _check(lib().gs_serialize(self._h, buf, ln.value, ctypes.byref(ln)))
        return buf.raw[: ln.value]

    def deserialize(self, data):
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        _check(lib().gs_deserialize(self._h, buf, len(data)))

    # --- delta (multi-GPU exchange)
    def set_delta_tracking(self, on=True):
        _check(lib().gs_set_delta_tracking(self._h, 1 if on else 0))

    # --- per-window change emission (sinks)
    def set_change_tracking(self, on=True):
        _check(lib().gs_set_change_tracking(self._h, 1 if on else 0))

    def take_changes_device(self, v, label, parity=None):
        """Rows (v, canonical label[, parity]) of every vertex inserted or relabelled
        since the previous take into DEVICE arrays (capacity >= num_vertices());
        returns the row count (gs_take_changes_device)."""
        n = _u64()
        cap = v.numel() if hasattr(v, "numel") else len(v)
        _check(lib().gs_take_changes_device(self._h, _ptr(v), _ptr(label), _ptr(parity), int(cap), ctypes.byref(n)))
        return n.value

    def take_changes(self):
        """take_changes_device into fresh device arrays; (v, label) numpy arrays."""
        import torch
        m = self.num_vertices() + 1
        dev = torch.device("cuda", self.device)
        v = torch.empty(m, dtype=torch.int64, device=dev)
        lab = torch.empty(m, dtype=torch.int64, device=dev)
        k = self.take_changes_device(v, lab)
        return v[:k].cpu().numpy(), lab[:k].cpu().numpy()

    def take_changes_host(self, with_parity=False):
        """gs_take_changes: the same rows into HOST arrays (what a JVM sink binds);
        (v, label[, parity]) numpy arrays."""
        import numpy as np
        m = self.num_vertices() + 1
        v = np.empty(m, dtype=np.int64)
        lab = np.empty(m, dtype=np.int64)
        par = np.empty(m, dtype=np.uint8) if with_parity else None
        n = _u64()
        _check(lib().gs_take_changes(self._h, v.ctypes.data, lab.ctypes.data,
                                     par.ctypes.data if with_parity else None, int(m), ctypes.byref(n)))
        k = n.value
        return (v[:k], lab[:k], par[:k]) if with_parity else (v[:k], lab[:k])

    def delta_capacity(self):
        """Rows the delta list holds between two takes / stages (gs_delta_capacity)."""
        n = _u64()
        _check(lib().gs_delta_capacity(self._h, ctypes.byref(n)))
        return n.value

    def take_delta_records(self, rec, cap, count):
        """Pack the delta since the last take into `rec` (device int64 [cap, 3]) and
        its record count into `count` (device int64 [1]); asynchronous on self.stream."""
        _check(lib().gs_take_delta_records(self._h, _ptr(rec), int(cap), _ptr(count)))

    def fold_take(self, src, dst, n, rec, cap, count):
        """One latency-path window (gs_fold_take_device): fold n device edges (tracked),
        take the records since the previous take into `rec` (device int64 [cap, 3]) and
        their count into `count` (device int64 [1]); returns the count once the window
        is complete. The full count word (| FAIL_BIT once a signed verdict failed) is
        kept in `last_take_word`: replay it with fold_records(rec, last_take_word)."""
        c = _u64()
        _check(lib().gs_fold_take_device(self._h, _ptr(src), _ptr(dst), int(n), _ptr(rec), int(cap), _ptr(count),
                                         ctypes.byref(c)))
        self.last_take_word = c.value
        return c.value & (FAIL_BIT - 1)

    def set_window_server(self, on=True):
        """gs_set_window_server: fold_take windows (<= 2^16 edges) go to one resident
        launch instead of a launch each."""
        _check(lib().gs_set_window_server(self._h, 1 if on else 0))

    def set_batch_dedup(self, on=True):
        """gs_set_batch_dedup: exact repeats of an edge within a fold's chunk are dropped
        by a hashing pre-pass before the fold (identical result)."""
        _check(lib().gs_set_batch_dedup(self._h, 1 if on else 0))

    def window_server_stats(self):
        a, b = _u64(), _u64()
        _check(lib().gs_window_server_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return {"launches": a.value, "windows": b.value}

    def delta_stage(self, send, cap, count, width=3):
        """Stage every pending record into `send` (device int64 [cap, width]) and the
        count word (| 2^62 when a signed verdict failed) into `count` (device int64
        [1]); asynchronous on self.stream. cap >= delta_capacity()."""
        _check(lib().gs_delta_stage(self._h, _ptr(send), int(cap), int(width), _ptr(count)))

    def fold_exchange(self, recv, counts, world, rows, skip_rank, width=3):
        """Fold a gathered exchange buffer: `world` blocks of `rows` rows of `width`
        int64, block r live for its first counts[r] rows (device count words),
        skipping block `skip_rank`."""
        _check(lib().gs_fold_exchange_device(self._h, _ptr(recv), _ptr(counts), int(world), int(rows), int(width),
                                             int(skip_rank)))

    def fold_records(self, rec, n, track=False):
        """Fold n device records {a, b, w} (another replica's delta). n may be a take's
        count word: FAIL_BIT ANDs a failed verdict into this summary."""
        _check(lib().gs_fold_records_device(self._h, _ptr(rec), int(n), 1 if track else 0))

    def fold_records_counted(self, rec, cap, count, track=False):
        """Replay a take with its count word read on the device (`count`: device int64
        [1] as the take wrote it; at most `cap` rows): no host round trip."""
        _check(lib().gs_fold_records_counted_device(self._h, _ptr(rec), int(cap), _ptr(count), 1 if track else 0))

    # --- introspection
    def set_profiling(self, on=True):
        _check(lib().gs_set_profiling(self._h, 1 if on else 0))

    def fold_text(self, text, sep=SEP_WHITESPACE):
        """gs_fold_text: parse edge lines from host bytes (reference source-map
        semantics, include/gs_ingest.h) and fold them. Returns the edge count;
        raises GSError(GS_ERR_PARSE) naming the first malformed line."""
        text = bytes(text)
        n = _u64()
        bad = _i64(-1)
        _check(lib().gs_fold_text(self._h, text, len(text), int(sep), ctypes.byref(n), ctypes.byref(bad)))
        return n.value

    def set_pipelining(self, depth=2):
        """gs_set_pipelining: depth 2 lets consecutive device folds overlap on the
        device (pipelined windows); any read orders behind them."""
        _check(lib().gs_set_pipelining(self._h, int(depth)))

    def set_hot_index(self, log2_entries=0, first_after_edges=0, rebuild_every_folds=1):
        """gs_set_hot_index: the plain CC fold's index of frequent ids. log2_entries < 0 turns it
        off, 0 restores the defaults (on for tables of at least 256 MiB), 1..20 forces an index
        of at most 2^log2_entries ids (two per 16-byte bucket) whatever the table's size, first
        built after first_after_edges edges and then every rebuild_every_folds folds."""
        _check(lib().gs_set_hot_index(self._h, int(log2_entries), int(first_after_edges), int(rebuild_every_folds)))

    def hot_index_stats(self):
        """gs_hot_index_stats: builds queued, ids the live index holds (entries), log2 of the ids
        it can hold (0: none), refreshes queued."""
        a = (_u64 * 4)()
        _check(lib().gs_hot_index_stats(self._h, a))
        return dict(zip(("builds", "entries", "log2_entries", "refreshes"), list(a)))

    def kernel_stats(self, name):
        n = _u64()
        ms = ctypes.c_double()
        _check(lib().gs_kernel_stats(self._h, KERNEL_IDS[name], ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def counters(self):
        """Device counters (gs_counters): vertices, failed, err, ovf, sent,
        hooks / hook iterations / failed CASes (debug build only)."""
        a = (_u64 * 8)()
        _check(lib().gs_counters(self._h, a))
        keys = ("vertices", "failed", "err", "ovf", "sent", "hooks", "hook_iters", "cas_fail")
        return dict(zip(keys, list(a)))

    def debug_counters(self):
        """Fold diagnostics (gs_debug_counters; debug build only, zeros otherwise)."""
        a = (_u64 * 16)()
        _check(lib().gs_debug_counters(self._h, a, 16))
        keys = ("edges", "key_cas", "key_cas_lost", "ttas", "shortcut", "same_root", "find_loads", "hooks_ok",
                "extra_probes", "hot_hits", "hot_fallbacks")
        return dict(zip(keys, list(a)))

    def table_capacity(self):
        n = _u64()
        _check(lib().gs_table_capacity(self._h, ctypes.byref(n)))
        return n.value

    def capacity_stats(self):
        """(waits, syncs, wait_ms) of the host capacity checks (gs_capacity_stats)."""
        w, s_ = _u64(), _u64()
        ms = ctypes.c_double()
        _check(lib().gs_capacity_stats(self._h, ctypes.byref(w), ctypes.byref(s_), ctypes.byref(ms)))
        return {"waits": w.value, "syncs": s_.value, "wait_ms": ms.value}


# ---------------------------------------------------------------- degree summary
class Degrees(_ResetHandle):
    """Streaming vertex degrees and their distribution (GS_KIND_DEGREE; the gs_degree_*
    section of include/gs_summary.h): SimpleEdgeStream.getDegrees / getInDegrees /
    getOutDegrees for direction "all" / "in" / "out", with optional edge deletions
    (example/DegreeDistribution.java). Owns a gs_handle."""

    _PREFIX = "gs"

    DIRECTIONS = {"all": DEGREE_ALL, "in": DEGREE_IN, "out": DEGREE_OUT}

    def __init__(self, direction="all", device=0, capacity_hint=1 << 20):
        self.dir = self.DIRECTIONS[direction] if isinstance(direction, str) else int(direction)
        self.device = device
        h = _vp()
        _check(lib().gs_create(ctypes.byref(h), device, KIND_DEGREE, capacity_hint))
        self._h = h

    def num_vertices(self):
        """Table entries: every vertex ever collected, those whose net count is <= 0 included."""
        n = _u64()
        _check(lib().gs_num_vertices(self._h, ctypes.byref(n)))
        return n.value

    def table_capacity(self):
        n = _u64()
        _check(lib().gs_table_capacity(self._h, ctypes.byref(n)))
        return n.value

    # --- fold / combine
    def fold(self, src, dst, deletions=None):
        """Fold host edges (int64 arrays); deletions: optional uint8 per edge, bit 0 = deletion."""
        s, d = _edges(src, dst)
        e = None
        if deletions is not None:
            e = np.ascontiguousarray(np.asarray(deletions, dtype=np.uint8))
            assert e.shape == s.shape
        _check(lib().gs_degree_fold(self._h, s.ctypes.data, d.ctypes.data, _ptr(e), len(s), self.dir))

    def fold_device(self, src, dst, n=None, stride=1, deletions=None, after=None):
        """Fold device-resident edges (torch tensors on this device or raw pointers), queued on
        the summary's stream; `after`: a stream the edges were written on (Summary.fold_device)."""
        if n is None:
            n = src.numel() // (stride if stride > 1 else 1)
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_degree_fold_device(self._h, _ptr(src), _ptr(dst), _ptr(deletions), int(n), int(stride),
                                           self.dir))

    def combine(self, other):
        """self += other (other unchanged)."""
        _check(lib().gs_combine(self._h, other._h))

    def serialize(self):
        ln = _sz()
        _check(lib().gs_serialize(self._h, None, 0, ctypes.byref(ln)))
        buf = ctypes.create_string_buffer(max(ln.value, 1))
        _check(lib().gs_serialize(self._h, buf, ln.value, ctypes.byref(ln)))
        return buf.raw[: ln.value]

    def deserialize(self, data):
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        _check(lib().gs_deserialize(self._h, buf, len(data)))

    # --- queries
    def find_device(self, v, degree, found=None, n=None):
        """degree[i] = degree of the DEVICE id v[i] (0 when absent), found[i] = 1 when > 0.
        Asynchronous on self.stream."""
        n = v.numel() if n is None else n
        _check(lib().gs_degree_find_device(self._h, _ptr(v), int(n), _ptr(degree), _ptr(found)))

    def degrees(self, sorted=True):
        """(vertex, degree) numpy int64 arrays of the vertices with degree > 0; sorted: ascending
        by vertex (on the device)."""
        got = _sz()
        n = max(self.num_vertices(), 1)  # the rows are a subset of the table entries
        v = np.empty(n, np.int64)
        d = np.empty(n, np.int64)
        _check(lib().gs_degree_export(self._h, v.ctypes.data, d.ctypes.data, n, ctypes.byref(got),
                                      1 if sorted else 0))
        return v[: got.value].copy(), d[: got.value].copy()

    def degrees_device(self, v, degree, sorted=False):
        """The same rows into DEVICE arrays (capacity v.numel()); returns the row count."""
        got = _sz()
        cap = v.numel() if hasattr(v, "numel") else len(v)
        _check(lib().gs_degree_export_device(self._h, _ptr(v), _ptr(degree), cap, ctypes.byref(got),
                                             1 if sorted else 0))
        return got.value

    def distribution(self):
        """(degree, count) numpy int64 arrays: the distinct degrees ascending and the number of
        vertices of each (the final state of DegreeDistributionMap)."""
        got = _sz()
        n = max(self.num_vertices(), 1)  # at most one distinct degree per vertex
        d = np.empty(n, np.int64)
        c = np.empty(n, np.int64)
        _check(lib().gs_degree_distribution(self._h, d.ctypes.data, c.ctypes.data, n, ctypes.byref(got)))
        return d[: got.value].copy(), c[: got.value].copy()

    def distribution_device(self, degree, count):
        """The distribution into DEVICE int64 arrays (capacity degree.numel()); returns its length."""
        got = _sz()
        cap = degree.numel() if hasattr(degree, "numel") else len(degree)
        _check(lib().gs_degree_distribution_device(self._h, _ptr(degree), _ptr(count), cap, ctypes.byref(got)))
        return got.value


# ---------------------------------------------------------------- triangle summary
class Triangles(_ResetHandle):
    """Exact triangle counts of a streamed graph (the gs_triangle_* section of
    include/gs_summary.h): the count of each window's graph (example/WindowTriangles: `window`)
    or the running global and per-vertex counts of an insertion-only stream
    (example/ExactTriangleCount: `fold` after `fold`). Direction, repeated edges and self-loops
    do not change the graph. `reset`: the graph empty and every counter zero; capacity is kept.
    Owns a gs_triangles handle. (SlidingTriangles is this class with removal.)"""

    _PREFIX = "gs_triangle"

    def __init__(self, device=0, edge_hint=1 << 20):
        self.device = device
        h = _vp()
        _check(lib().gs_triangle_create(ctypes.byref(h), device, int(edge_hint)))
        self._h = h

    def fold(self, src, dst):
        """Fold host edges (int64 arrays)."""
        s, d = _edges(src, dst)
        _check(lib().gs_triangle_fold(self._h, s.ctypes.data, d.ctypes.data, len(s)))

    def fold_device(self, src, dst, n=None, stride=1, after=None):
        """Fold device-resident edges (torch tensors on this device or raw pointers), queued on
        the handle's stream; `after`: a stream the edges were written on (Degrees.fold_device).
        The fold synchronises with the host once (the number of new edges)."""
        if n is None:
            n = src.numel() // (stride if stride > 1 else 1)
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_triangle_fold_device(self._h, _ptr(src), _ptr(dst), int(n), int(stride)))

    def count(self):
        """(triangles, edges, vertices) of the graph folded so far. Synchronises."""
        t, e, v = _u64(), _u64(), _u64()
        _check(lib().gs_triangle_count(self._h, ctypes.byref(t), ctypes.byref(e), ctypes.byref(v)))
        return t.value, e.value, v.value

    def count_device(self, out):
        """The same three 64-bit words into DEVICE memory; asynchronous on self.stream."""
        _check(lib().gs_triangle_count_device(self._h, _ptr(out)))

    def find_device(self, v, count, found=None, n=None):
        """count[i] = triangles through the DEVICE id v[i] (0 when absent), found[i] = 1 when
        v[i] is a vertex of the graph. Asynchronous on self.stream."""
        n = v.numel() if n is None else n
        _check(lib().gs_triangle_find_device(self._h, _ptr(v), int(n), _ptr(count), _ptr(found)))

    def local_counts(self, nonzero_only=False):
        """(vertex, triangles through it) numpy int64 arrays, ascending by vertex."""
        got = _sz()
        n = max(self.count()[2], 1)
        v = np.empty(n, np.int64)
        c = np.empty(n, np.int64)
        _check(lib().gs_triangle_export(self._h, v.ctypes.data, c.ctypes.data, n, ctypes.byref(got),
                                        1 if nonzero_only else 0))
        return v[: got.value].copy(), c[: got.value].copy()

    def local_counts_device(self, v, count, nonzero_only=False):
        """The same rows into DEVICE arrays (capacity v.numel()); returns the row count."""
        got = _sz()
        cap = v.numel() if hasattr(v, "numel") else len(v)
        _check(lib().gs_triangle_export_device(self._h, _ptr(v), _ptr(count), cap, ctypes.byref(got),
                                               1 if nonzero_only else 0))
        return got.value

    def window(self, src, dst):
        """The triangle count of the graph of one window of host edges: reset, fold, count."""
        self.reset()
        self.fold(src, dst)
        return self.count()[0]

    def stats(self):
        """gs_testing_triangle_stats: intersection steps and the longest row met since reset, and
        the phase times (microseconds) of the last fold under testing(triangle_profile=1)."""
        out = (_u64 * 6)()
        _check(lib().gs_testing_triangle_stats(self._h, out))
        return {"steps": out[0], "hot_row": out[1], "canon_us": out[2], "sort_dedup_us": out[3], "merge_us": out[4],
                "count_us": out[5]}

    def bins(self):
        """gs_testing_triangle_bins: (wave, workgroup), the new edges the count step of the last
        fold with new edges gave to a wave and to a workgroup; (0, 0) under triangle_variant 1."""
        out = (_u64 * 2)()
        _check(lib().gs_testing_triangle_bins(self._h, out))
        return out[0], out[1]


class SlidingTriangles(Triangles):
    """Triangles whose edges also leave the graph: by name (`remove`) or by age in folds
    (`expire`; `slide` is one step of a sliding window). The same gs_triangles handle and every
    method of Triangles; the answers always equal those of a fresh handle that folded exactly
    the surviving edges, and a vertex without edges is no vertex any more. `refresh=True`
    (gs_triangle_set_refresh): an edge that a fold contains again takes that fold's age. The
    pinned public surface of Triangles itself stays as it was, so the removal lives here."""

    def __init__(self, device=0, edge_hint=1 << 20, refresh=False):
        super().__init__(device, edge_hint)
        if refresh:
            _check(lib().gs_triangle_set_refresh(self._h, 1))

    def remove(self, src, dst):
        """Remove host pairs (int64 arrays) from the graph; pairs it does not hold, loops and
        repeats change nothing."""
        s, d = _edges(src, dst)
        _check(lib().gs_triangle_remove(self._h, s.ctypes.data, d.ctypes.data, len(s)))

    def remove_device(self, src, dst, n=None, stride=1, after=None):
        """Remove device-resident pairs, queued on the handle's stream as fold_device queues a
        fold. Synchronises with the host once (the number of dying edges)."""
        if n is None:
            n = src.numel() // (stride if stride > 1 else 1)
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_triangle_remove_device(self._h, _ptr(src), _ptr(dst), int(n), int(stride)))

    def expire(self, folds):
        """Remove every edge older than the last `folds` folds (folds >= 1; a fold of no edges
        counts as a fold)."""
        _check(lib().gs_triangle_expire(self._h, int(folds)))

    def slide(self, src, dst, panes):
        """One step of a window that slides by a pane of host edges: fold the pane, expire what
        is older than `panes` panes, return the triangle count. With refresh=True the graph is
        the union of the last `panes` panes."""
        self.fold(src, dst)
        self.expire(panes)
        return self.count()[0]

    def remove_stats(self):
        """gs_testing_triangle_remove_stats: the last removal (remove, remove_device, expire)."""
        out = (_u64 * 8)()
        _check(lib().gs_testing_triangle_remove_stats(self._h, out))
        keys = ("edges_removed", "triangles_destroyed", "vertices_vanished", "wave_list", "workgroup_list", "steps",
                "table_slots", "entries")
        return dict(zip(keys, (int(x) for x in out)))


# ---------------------------------------------------------------- window slices
class Slice(_Handle):
    """The per-vertex neighbourhoods of one window of (src, dst, value) edges (the gs_slice_*
    section of include/gs_summary.h: SimpleEdgeStream.slice and its SnapshotStream): `window`
    replaces the handle's window, `reduce` gives one value per vertex (reduceOnEdges),
    `neighborhoods` the CSR that foldNeighbors / applyOnNeighbors iterate, entries in arrival
    order. Nothing is deduplicated. Owns a gs_slices handle."""

    _PREFIX = "gs_slice"

    def __init__(self, device=0, edge_hint=0):
        self.device = device
        h = _vp()
        _check(lib().gs_slice_create(ctypes.byref(h), device, int(edge_hint)))
        self._h = h
        self._has_val = True  # the current window carries values (an empty one reads none)

    def window(self, src, dst, val=None, direction="out"):
        """One window of host edges (int64 arrays; val None: a stream without values)."""
        s, d = _edges(src, dst)
        w = None
        if val is not None:
            w = _int64s(val)
            assert w.shape == s.shape
        _check(lib().gs_slice_window(self._h, s.ctypes.data, d.ctypes.data, None if w is None else w.ctypes.data,
                                     len(s), _slice_dir(direction)))
        self._has_val = w is not None or len(s) == 0

    def window_device(self, src, dst, val=None, direction="out", n=None, stride=1, after=None):
        """One window of device-resident edges (torch tensors on this device or raw pointers),
        element i at index i * stride; `after`: a stream the edges were written on. The call
        synchronises with the host once (the vertex count)."""
        if n is None:
            n = src.numel() // (stride if stride > 1 else 1)
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_slice_window_device(self._h, _ptr(src), _ptr(dst), _ptr(val), int(n), int(stride),
                                            _slice_dir(direction)))
        self._has_val = val is not None or int(n) == 0

    def size(self):
        """(vertices, entries) of the current window."""
        v, e = _u64(), _u64()
        _check(lib().gs_slice_size(self._h, ctypes.byref(v), ctypes.byref(e)))
        return v.value, e.value

    def reduce(self, op="sum"):
        """(vertex, value) numpy int64 arrays, ascending by vertex; op: sum (wraps), min, max, count."""
        n = max(self.size()[0], 1)
        got = _sz()
        v = np.empty(n, np.int64)
        out = np.empty(n, np.int64)
        _check(lib().gs_slice_reduce(self._h, _slice_op(op), v.ctypes.data, out.ctypes.data, n, ctypes.byref(got)))
        return v[: got.value].copy(), out[: got.value].copy()

    def reduce_device(self, op, v, out):
        """The same rows into DEVICE arrays (capacity v.numel()), queued on self.stream; returns
        the row count."""
        got = _sz()
        cap = v.numel() if hasattr(v, "numel") else len(v)
        _check(lib().gs_slice_reduce_device(self._h, _slice_op(op), _ptr(v), _ptr(out), cap, ctypes.byref(got)))
        return got.value

    def neighborhoods(self):
        """(vertex[nv], offset[nv + 1], neighbor[ne], val[ne]) numpy arrays: vertices ascending,
        the entries of vertex k at offset[k] .. offset[k + 1] - 1 in arrival order; val is None
        for a window without values."""
        nv, ne = self.size()
        got_v, got_e = _sz(), _sz()
        v = np.empty(max(nv, 1), np.int64)
        off = np.zeros(max(nv, 1) + 1, np.uint64)
        nb = np.empty(max(ne, 1), np.int64)
        w = np.empty(max(ne, 1), np.int64) if self._has_val else None
        _check(lib().gs_slice_neighborhoods(self._h, v.ctypes.data, off.ctypes.data, nb.ctypes.data,
                                            None if w is None else w.ctypes.data, len(v), len(nb),
                                            ctypes.byref(got_v), ctypes.byref(got_e)))
        nv, ne = got_v.value, got_e.value
        return v[:nv].copy(), off[: nv + 1].copy(), nb[:ne].copy(), None if w is None else w[:ne].copy()

    def neighborhoods_device(self, v, offset, neighbor, val=None):
        """The CSR into DEVICE arrays (capacities v.numel() and neighbor.numel(); offset holds
        v.numel() + 1 words), queued on self.stream; returns (vertices, entries)."""
        got_v, got_e = _sz(), _sz()
        cap_v = v.numel() if hasattr(v, "numel") else len(v)
        cap_e = neighbor.numel() if hasattr(neighbor, "numel") else len(neighbor)
        _check(lib().gs_slice_neighborhoods_device(self._h, _ptr(v), _ptr(offset), _ptr(neighbor), _ptr(val), cap_v,
                                                   cap_e, ctypes.byref(got_v), ctypes.byref(got_e)))
        return got_v.value, got_e.value

    def stats(self):
        """gs_testing_slice_stats: tiles of the last reduce, tiles of the window without a head
        (carry records that hand a run on), the longest segment, and the phase times
        (microseconds) of the last calls under testing(slice_profile=1)."""
        out = (_u64 * 8)()
        _check(lib().gs_testing_slice_stats(self._h, out))
        return {"tiles": out[0], "headless_tiles": out[1], "longest": out[2], "expand_us": out[3], "sort_us": out[4],
                "heads_us": out[5], "reduce_us": out[6], "gather_us": out[7]}


def _slice_dir(direction):
    return SLICE_DIRECTIONS[direction] if isinstance(direction, str) else int(direction)


def _slice_op(op):
    return SLICE_OPS[op] if isinstance(op, str) else int(op)


# ---------------------------------------------------------------- distinct streams
class Distinct(_ResetHandle):
    """The first-seen edges and vertices of an edge stream (the gs_distinct_* section of
    include/gs_summary.h: SimpleEdgeStream.distinct and getVertices): `fold` answers which edges
    and endpoint entries of a batch are seen for the first time, always keeping the arrival-first
    occurrence; `vertices` lists every vertex in first-appearance (rank) order and `edges` every
    edge by first arrival. mode: "directed" keys an edge by (src, dst), "undirected" by the
    unordered pair. `reset`: both sets empty and folded = 0; capacity is kept. Owns a gs_distinct
    handle."""

    _PREFIX = "gs_distinct"

    def __init__(self, device=0, mode="directed", vertex_hint=0, edge_hint=0):
        self.device = device
        self.mode = _distinct_mode(mode)
        h = _vp()
        _check(lib().gs_distinct_create(ctypes.byref(h), device, self.mode, int(vertex_hint), int(edge_hint)))
        self._h = h

    def fold(self, src, dst):
        """Fold host edges (int64 arrays); returns (new_vertices, new_edges) of this fold."""
        s, d = _edges(src, dst)
        _check(lib().gs_distinct_fold(self._h, s.ctypes.data, d.ctypes.data, len(s)))
        return self.size()[3:]

    def fold_device(self, src, dst, n=None, stride=1, after=None):
        """Fold device-resident edges (torch tensors on this device or raw pointers), element i
        at index i * stride; `after`: a stream the edges were written on. The fold synchronises
        with the host once (the two new counts); returns (new_vertices, new_edges)."""
        if n is None:
            n = src.numel() // (stride if stride > 1 else 1)
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_distinct_fold_device(self._h, _ptr(src), _ptr(dst), int(n), int(stride)))
        return self.size()[3:]

    def size(self):
        """(vertices, edges, folded, new_vertices, new_edges): totals and the last fold's counts."""
        w = [_u64() for _ in range(5)]
        _check(lib().gs_distinct_size(self._h, *[ctypes.byref(x) for x in w]))
        return tuple(x.value for x in w)

    def new_edges(self):
        """(index, src, dst) of the last fold's new edges: index (uint32) ascending, the edges
        with the orientation they arrived with."""
        n = max(self.size()[4], 1)
        got = _sz()
        idx = np.empty(n, np.uint32)
        s = np.empty(n, np.int64)
        d = np.empty(n, np.int64)
        _check(lib().gs_distinct_new_edges(self._h, idx.ctypes.data, s.ctypes.data, d.ctypes.data, n,
                                           ctypes.byref(got)))
        return idx[: got.value].copy(), s[: got.value].copy(), d[: got.value].copy()

    def new_edges_device(self, index, src=None, dst=None, cap=None):
        """The same rows into DEVICE arrays (each may be None; capacity: `cap`, or the first
        array's numel), queued on self.stream; returns the row count."""
        got = _sz()
        _check(lib().gs_distinct_new_edges_device(self._h, _ptr(index), _ptr(src), _ptr(dst),
                                                  _cap_of(cap, index, src, dst), ctypes.byref(got)))
        return got.value

    def new_vertices(self):
        """(v, entry) of the last fold's new vertices: entry (uint32) ascending; entry 2i is the
        src and 2i + 1 the dst of edge i of the fold."""
        n = max(self.size()[3], 1)
        got = _sz()
        v = np.empty(n, np.int64)
        e = np.empty(n, np.uint32)
        _check(lib().gs_distinct_new_vertices(self._h, v.ctypes.data, e.ctypes.data, n, ctypes.byref(got)))
        return v[: got.value].copy(), e[: got.value].copy()

    def new_vertices_device(self, v, entry=None, cap=None):
        got = _sz()
        _check(lib().gs_distinct_new_vertices_device(self._h, _ptr(v), _ptr(entry), _cap_of(cap, v, entry),
                                                     ctypes.byref(got)))
        return got.value

    def vertices(self):
        """Every vertex in rank (first-appearance) order, a numpy int64 array."""
        n = max(self.size()[0], 1)
        got = _sz()
        v = np.empty(n, np.int64)
        _check(lib().gs_distinct_vertices(self._h, v.ctypes.data, n, ctypes.byref(got)))
        return v[: got.value].copy()

    def vertices_device(self, v, cap=None):
        got = _sz()
        _check(lib().gs_distinct_vertices_device(self._h, _ptr(v), _cap_of(cap, v), ctypes.byref(got)))
        return got.value

    def edges(self):
        """(src, dst, first): every edge ascending by first arrival, first (uint64) = that
        arrival number in the whole stream."""
        n = max(self.size()[1], 1)
        got = _sz()
        s = np.empty(n, np.int64)
        d = np.empty(n, np.int64)
        f = np.empty(n, np.uint64)
        _check(lib().gs_distinct_edges(self._h, s.ctypes.data, d.ctypes.data, f.ctypes.data, n, ctypes.byref(got)))
        return s[: got.value].copy(), d[: got.value].copy(), f[: got.value].copy()

    def edges_device(self, src, dst=None, first=None, cap=None):
        got = _sz()
        _check(lib().gs_distinct_edges_device(self._h, _ptr(src), _ptr(dst), _ptr(first),
                                              _cap_of(cap, src, dst, first), ctypes.byref(got)))
        return got.value

    def rank_device(self, v, rank, found=None, n=None):
        """rank[i] = first-appearance rank of the DEVICE id v[i], -1 when absent; found[i] = 1
        when present. Asynchronous on self.stream."""
        n = v.numel() if n is None else n
        _check(lib().gs_distinct_rank_device(self._h, _ptr(v), int(n), _ptr(rank), _ptr(found)))

    def contains_device(self, src, dst, found, n=None):
        """found[i] = 1 when the DEVICE pair (src[i], dst[i]) is in the edge set (either
        orientation in undirected mode). Asynchronous on self.stream."""
        n = src.numel() if n is None else n
        _check(lib().gs_distinct_contains_device(self._h, _ptr(src), _ptr(dst), int(n), _ptr(found)))

    def stats(self):
        """gs_testing_distinct_stats: table slots, rebuilds since create, the longest probe and
        the edge-compaction tiles of the last fold."""
        out = (_u64 * 6)()
        _check(lib().gs_testing_distinct_stats(self._h, out))
        return {"vertex_slots": out[0], "edge_slots": out[1], "vertex_rebuilds": out[2], "edge_rebuilds": out[3],
                "longest_probe": out[4], "tiles": out[5]}

    def phases(self):
        """gs_testing_distinct_phases: the last fold under testing(distinct_profile=1): the phase
        times (microseconds), the occurrences that issued an atomic and all its occurrences."""
        out = (_u64 * 7)()
        _check(lib().gs_testing_distinct_phases(self._h, out))
        return {"vertex_probe_us": out[0], "vertex_compact_us": out[1], "edge_probe_us": out[2],
                "edge_compact_us": out[3], "control_us": out[4], "atomics": out[5], "occurrences": out[6]}


def _distinct_mode(mode):
    return DISTINCT_MODES[mode] if isinstance(mode, str) else int(mode)


def _cap_of(cap, *arrays):
    if cap is not None:
        return int(cap)
    for a in arrays:
        if a is not None and not isinstance(a, int):
            return a.numel() if hasattr(a, "numel") else len(a)
    return 0


# ---------------------------------------------------------------- k-spanner summary
class Spanner(_ResetHandle):
    """The streaming k-spanner of library/Spanner.java (the gs_spanner_* section of
    include/gs_summary.h): an arriving edge is accepted into the graph iff its endpoints are more
    than k edges apart in the graph the edges before it left, exactly in arrival order however
    the stream is cut into folds. `reset`: the graph empty; capacity and k are kept. Owns a
    gs_spanner handle."""

    _PREFIX = "gs_spanner"

    def __init__(self, k=3, device=0, edge_hint=1 << 16):
        self.device = device
        self.k = int(k)
        h = _vp()
        _check(lib().gs_spanner_create(ctypes.byref(h), device, int(k), int(edge_hint)))
        self._h = h

    def fold(self, src, dst):
        """Fold host edges (int64 arrays) in arrival order; returns the accepted mask (bool)."""
        s, d = _edges(src, dst)
        acc = np.zeros(len(s), np.uint8)
        _check(lib().gs_spanner_fold(self._h, s.ctypes.data, d.ctypes.data, len(s), acc.ctypes.data))
        return acc.astype(bool)

    def fold_device(self, src, dst, accepted=None, n=None, stride=1, after=None):
        """Fold device-resident edges (torch tensors on this device or raw pointers); `accepted`
        (optional): a DEVICE uint8 tensor of n bytes, written on the handle's stream; `after`: a
        stream the edges were written on. The fold synchronises with the host."""
        if n is None:
            n = src.numel() // (stride if stride > 1 else 1)
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_spanner_fold_device(self._h, _ptr(src), _ptr(dst), int(n), _ptr(accepted), int(stride)))

    def add(self, src, dst):
        """AdjacencyListGraph.addEdge for host edges: each joins the graph unless it is there."""
        s, d = _edges(src, dst)
        _check(lib().gs_spanner_add(self._h, s.ctypes.data, d.ctypes.data, len(s)))

    def within(self, src, dst, k=None):
        """boundedBFS(src[i], dst[i], k) on the graph as it stands, host arrays; bool array."""
        s, d = _edges(np.atleast_1d(src), np.atleast_1d(dst))
        out = np.zeros(len(s), np.uint8)
        _check(lib().gs_spanner_within(self._h, s.ctypes.data, d.ctypes.data, len(s),
                                       self.k if k is None else int(k), out.ctypes.data))
        return out.astype(bool)

    def within_device(self, src, dst, out, k=None, n=None):
        """The same for DEVICE ids into the DEVICE uint8 tensor `out`, queued on self.stream."""
        n = src.numel() if n is None else n
        _check(lib().gs_spanner_within_device(self._h, _ptr(src), _ptr(dst), int(n),
                                              self.k if k is None else int(k), _ptr(out)))

    def combine(self, other):
        """CombineSpanners: other's edges, ascending by (lo, hi), folded into this spanner with
        this spanner's k; `other` is unchanged."""
        _check(lib().gs_spanner_combine(self._h, other._h))

    def count(self):
        """(edges, vertices) of the graph. Synchronises."""
        e, v = _u64(), _u64()
        _check(lib().gs_spanner_count(self._h, ctypes.byref(e), ctypes.byref(v)))
        return e.value, v.value

    def edges(self):
        """(lo, hi) numpy int64 arrays: the spanner's edges ascending by (lo, hi)."""
        got = _sz()
        n = max(self.count()[0], 1)
        lo = np.empty(n, np.int64)
        hi = np.empty(n, np.int64)
        _check(lib().gs_spanner_export(self._h, lo.ctypes.data, hi.ctypes.data, n, ctypes.byref(got)))
        return lo[: got.value].copy(), hi[: got.value].copy()

    def edges_device(self, lo, hi):
        """The same rows into DEVICE arrays (capacity lo.numel()); returns the edge count."""
        got = _sz()
        cap = lo.numel() if hasattr(lo, "numel") else len(lo)
        _check(lib().gs_spanner_export_device(self._h, _ptr(lo), _ptr(hi), cap, ctypes.byref(got)))
        return got.value

    def neighbors(self):
        """The adjacency as a CSR of numpy arrays (v, offset, neighbor): vertices ascending, the
        neighbours of v[i] = neighbor[offset[i]:offset[i + 1]] ascending (getAdjacencyMap())."""
        e, nv = self.count()
        v = np.empty(max(nv, 1), np.int64)
        off = np.zeros(max(nv, 1) + 1, np.uint64)
        nb = np.empty(max(2 * e, 1), np.int64)
        gv, ge = _sz(), _sz()
        _check(lib().gs_spanner_neighbors(self._h, v.ctypes.data, off.ctypes.data, nb.ctypes.data, len(v), len(nb),
                                          ctypes.byref(gv), ctypes.byref(ge)))
        return v[: gv.value].copy(), off[: gv.value + 1].astype(np.int64), nb[: ge.value].copy()

    def stats(self):
        """gs_testing_spanner_stats: the last fold."""
        out = (_u64 * 6)()
        _check(lib().gs_testing_spanner_stats(self._h, out))
        return {"filter_drops": out[0], "pending": out[1], "rounds": out[2], "tail": out[3], "heavy": out[4],
                "longest_row": out[5]}

    def generation(self, set=None):
        """gs_testing_spanner_generation: the generations the heavy search's stamp arenas have
        used since their last clear; `set` moves the counter first (clamped to SPANNER_MAX_GEN)."""
        out = _u64()
        _check(lib().gs_testing_spanner_generation(self._h, -1 if set is None else int(set), ctypes.byref(out)))
        return out.value


# ---------------------------------------------------------------- weighted matching
class Matching(_ResetHandle):
    """The streaming greedy weighted matching of example/CentralizedWeightedMatching.java (the
    gs_matching_* section of include/gs_summary.h): an arriving edge (u, v, w) joins the matching
    M iff w > 2 * (the values of M's edges at u and v), in Java long arithmetic, and then removes
    them; exactly in arrival order however the stream is cut into folds. `reset`: M empty, no vertex
    seen, weight-safe again; capacity and tuning are kept. Owns a gs_matching handle."""

    _PREFIX = "gs_matching"

    def __init__(self, device=0, vertex_hint=1 << 16):
        self.device = device
        h = _vp()
        _check(lib().gs_matching_create(ctypes.byref(h), device, int(vertex_hint)))
        self._h = h

    def fold(self, src, dst, val):
        """Fold host arrivals (int64 arrays) in order; returns the accepted mask (bool)."""
        s, d = _edges(src, dst)
        w = _int64s(val)
        assert s.shape == w.shape
        acc = np.zeros(len(s), np.uint8)
        _check(lib().gs_matching_fold(self._h, s.ctypes.data, d.ctypes.data, w.ctypes.data, len(s), acc.ctypes.data))
        return acc.astype(bool)

    def fold_device(self, src, dst, val, accepted=None, n=None, stride=1, after=None):
        """Fold device-resident arrivals (torch tensors on this device or raw pointers), element i
        at index i * stride; `accepted` (optional): a DEVICE uint8 tensor of n bytes, written on
        the handle's stream; `after`: a stream the arrays were written on. The fold synchronises
        with the host."""
        if n is None:
            n = (src.numel() + stride - 1) // stride
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_matching_fold_device(self._h, _ptr(src), _ptr(dst), _ptr(val), int(n), _ptr(accepted),
                                             int(stride)))

    def events(self):
        """The last fold's MatchingEvent rows as numpy arrays (arrival uint32, type uint8 --
        MATCHING_EVENTS --, src, dst, val int64), ascending by arrival; an arrival's REMOVEs (the
        edge at its source endpoint first) precede its ADD."""
        got = _sz()
        rc = lib().gs_matching_events(self._h, None, None, None, None, None, 0, ctypes.byref(got))
        if rc != GS_ERR_TRUNCATED:  # (the row count of a fold with events)
            _check(rc)
        n = max(got.value, 1)
        a = np.empty(n, np.uint32)
        t = np.empty(n, np.uint8)
        s, d, w = (np.empty(n, np.int64) for _ in range(3))
        _check(lib().gs_matching_events(self._h, a.ctypes.data, t.ctypes.data, s.ctypes.data, d.ctypes.data,
                                        w.ctypes.data, n, ctypes.byref(got)))
        k = got.value
        return a[:k].copy(), t[:k].copy(), s[:k].copy(), d[:k].copy(), w[:k].copy()

    def events_device(self, arrival, type, src, dst, val):
        """The same rows into DEVICE arrays (capacity src.numel(); any may be None); returns the
        row count."""
        got = _sz()
        first = next(x for x in (src, dst, val, arrival, type) if x is not None)
        cap = first.numel() if hasattr(first, "numel") else len(first)
        _check(lib().gs_matching_events_device(self._h, _ptr(arrival), _ptr(type), _ptr(src), _ptr(dst), _ptr(val),
                                               cap, ctypes.byref(got)))
        return got.value

    def count(self):
        """(edges of M, distinct vertices seen, wrapping sum of M's values). No device call."""
        e, v, w = _u64(), _u64(), ctypes.c_int64()
        _check(lib().gs_matching_count(self._h, ctypes.byref(e), ctypes.byref(v), ctypes.byref(w)))
        return e.value, v.value, w.value

    def edges(self):
        """(src, dst, val, first) numpy arrays: M ascending by the global arrival number `first`
        at which each edge was accepted."""
        got = _sz()
        n = max(self.count()[0], 1)
        s, d, w = (np.empty(n, np.int64) for _ in range(3))
        f = np.empty(n, np.uint64)
        _check(lib().gs_matching_export(self._h, s.ctypes.data, d.ctypes.data, w.ctypes.data, f.ctypes.data, n,
                                        ctypes.byref(got)))
        k = got.value
        return s[:k].copy(), d[:k].copy(), w[:k].copy(), f[:k].copy()

    def edges_device(self, src, dst, val, first=None):
        """The same rows into DEVICE arrays (capacity src.numel()); returns the edge count."""
        got = _sz()
        cap = src.numel() if hasattr(src, "numel") else len(src)
        _check(lib().gs_matching_export_device(self._h, _ptr(src), _ptr(dst), _ptr(val), _ptr(first), cap,
                                               ctypes.byref(got)))
        return got.value

    def mate_device(self, v, mate, val, found, n=None):
        """Per DEVICE id v[i]: found[i] (uint8) = it is matched, mate[i] / val[i] = its partner in M
        and the edge's value (0 otherwise); queued on self.stream."""
        n = v.numel() if n is None else n
        _check(lib().gs_matching_mate_device(self._h, _ptr(v), int(n), _ptr(mate), _ptr(val), _ptr(found)))

    def stats(self):
        """gs_testing_matching_stats: the last fold."""
        out = (_u64 * 6)()
        _check(lib().gs_testing_matching_stats(self._h, out))
        return {"rounds": out[0], "iterations": out[1], "tail": out[2], "accepted": out[3], "fallbacks": out[4],
                "weight_safe": bool(out[5])}

    def tune(self, round_cap=None, iter_cap=None, sharpen=None):
        """gs_testing_matching_tune, per handle: round_cap (0: everything to the tail, huge: no
        tail), iter_cap (fixpoint passes per round), sharpen (False: off). A negative value (or
        sharpen=True) restores the product value; None leaves a control as it is."""
        if round_cap is not None:
            _check(lib().gs_testing_matching_tune(self._h, 0, int(round_cap)))
        if iter_cap is not None:
            _check(lib().gs_testing_matching_tune(self._h, 1, int(iter_cap)))
        if sharpen is not None:
            _check(lib().gs_testing_matching_tune(self._h, 2, -1 if sharpen else 1))


# ---------------------------------------------------------------- sampling triangle estimate
class TriangleSampler(_ResetHandle):
    """The sampling triangle estimate of example/BroadcastTriangleCount.java at parallelism 1 with
    the seeded coin of example/IncidenceSamplingTriangleCount.java (the gs_trisample_* section of
    include/gs_summary.h): `samples` instances each keep one candidate (src, trg, third), resampled
    at arrival t with probability 1/t by a coin that is exact to java.util.Random; the rows are
    (edge count, estimate, betaSum) whenever the estimate changes, the same however the stream is
    cut into folds. `reset`: no arrival folded, the generators reseeded; capacity and tuning are
    kept. Owns a gs_trisample handle."""

    _PREFIX = "gs_trisample"

    def __init__(self, samples=10000, vertices=1000, seed=-559038737, third_seed=0, device=0):
        self.device = device
        self.samples = int(samples)
        h = _vp()
        _check(lib().gs_trisample_create(ctypes.byref(h), device, int(samples), int(vertices), int(seed),
                                         int(third_seed) & ((1 << 64) - 1)))
        self._h = h

    def fold(self, src, dst):
        """Fold host arrivals (int64 arrays) in order; returns the fold's row count."""
        s, d = _edges(src, dst)
        rows = _sz()
        _check(lib().gs_trisample_fold(self._h, s.ctypes.data, d.ctypes.data, len(s), ctypes.byref(rows)))
        return rows.value

    def fold_device(self, src, dst, n=None, stride=1, after=None):
        """Fold device-resident arrivals (torch tensors on this device or raw pointers), element i
        at index i * stride; `after`: a stream the arrays were written on. The fold synchronises
        with the host; returns the fold's row count."""
        if n is None:
            n = (src.numel() + stride - 1) // stride
        if after is not None:
            self.wait_stream(after)
        rows = _sz()
        _check(lib().gs_trisample_fold_device(self._h, _ptr(src), _ptr(dst), int(n), int(stride), ctypes.byref(rows)))
        return rows.value

    def rows(self):
        """The last fold's rows as numpy int32 arrays (edges, estimate, beta_sum)."""
        got = _sz()
        rc = lib().gs_trisample_rows(self._h, None, None, None, 0, ctypes.byref(got))
        if rc != GS_ERR_TRUNCATED:  # (the row count of a fold with rows)
            _check(rc)
        n = max(got.value, 1)
        e, est, b = (np.empty(n, np.int32) for _ in range(3))
        _check(lib().gs_trisample_rows(self._h, e.ctypes.data, est.ctypes.data, b.ctypes.data, n, ctypes.byref(got)))
        k = got.value
        return e[:k].copy(), est[:k].copy(), b[:k].copy()

    def rows_device(self, edges, estimate, beta_sum):
        """The same rows into DEVICE int32 arrays (capacity of the first one given; any may be
        None); returns the row count."""
        got = _sz()
        first = next(x for x in (edges, estimate, beta_sum) if x is not None)
        cap = first.numel() if hasattr(first, "numel") else len(first)
        _check(lib().gs_trisample_rows_device(self._h, _ptr(edges), _ptr(estimate), _ptr(beta_sum), cap,
                                              ctypes.byref(got)))
        return got.value

    def estimate(self):
        """(arrivals folded, betaSum now, the last emitted estimate). No device call."""
        a, b, e = _u64(), ctypes.c_int32(), ctypes.c_int32()
        _check(lib().gs_trisample_estimate(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(e)))
        return a.value, b.value, e.value

    def states(self):
        """Every instance's candidate as numpy arrays (src, trg, third int64, flags uint8 -- bit 0
        srcEdgeFound, bit 1 trgEdgeFound, bit 2 beta --, sampled_at int32)."""
        s, t, th = (np.empty(self.samples, np.int64) for _ in range(3))
        f = np.empty(self.samples, np.uint8)
        at = np.empty(self.samples, np.int32)
        _check(lib().gs_trisample_states(self._h, s.ctypes.data, t.ctypes.data, th.ctypes.data, f.ctypes.data,
                                         at.ctypes.data))
        return s, t, th, f, at

    def states_device(self, src, trg, third, flags, sampled_at):
        """The same columns into DEVICE arrays of `samples` elements (any may be None); queued on
        self.stream."""
        _check(lib().gs_trisample_states_device(self._h, _ptr(src), _ptr(trg), _ptr(third), _ptr(flags),
                                                _ptr(sampled_at)))

    def stats(self):
        """gs_testing_trisample_stats: the last fold."""
        return self.phases()[0]

    def phases(self):
        """(stats, microseconds of the last fold's coin pass, sort and segments, search pass,
        outcomes and rows): the times are zero unless tune(profile=True)."""
        out = (_u64 * 8)()
        _check(lib().gs_testing_trisample_stats(self._h, out))
        return ({"coins": out[0], "segments": out[1], "max_attempts": out[2], "rows": out[3]},
                {"coin": out[4], "segments": out[5], "search": out[6], "rows": out[7]})

    def tune(self, chunk=None, tile=None, profile=None, keys=None, piece=None, edge_count=None):
        """gs_testing_trisample_tune, per handle: the arrivals per workgroup of the coin pass and
        of the search pass (at most TRISAMPLE_TILE), whether a fold times its phases, the most
        keys the resample list is first sized for, and the arrivals of one device piece of a fold
        (at most TRISAMPLE_MAX_FOLD; a longer fold keeps no rows). A value <= 0 restores the
        product value; None leaves a control as it is. `edge_count` is an action: it sets the
        arrivals folded so far (0 .. TRISAMPLE_MAX_ARRIVALS) and nothing else, after which the
        handle corresponds to no real stream -- only for tests right before the arrival limit."""
        if piece is not None:
            _check(lib().gs_testing_trisample_tune(self._h, 4, int(piece)))
        if edge_count is not None:
            _check(lib().gs_testing_trisample_tune(self._h, 5, int(edge_count)))
        if keys is not None:
            _check(lib().gs_testing_trisample_tune(self._h, 3, int(keys)))
        if profile is not None:
            _check(lib().gs_testing_trisample_tune(self._h, 2, 1 if profile else -1))
        if chunk is not None:
            _check(lib().gs_testing_trisample_tune(self._h, 0, int(chunk)))
        if tile is not None:
            _check(lib().gs_testing_trisample_tune(self._h, 1, int(tile)))


# ---------------------------------------------------------------- degree streams
class DegreeStream(_ResetHandle):
    """Every running degree and every distribution record of an edge stream (the gs_degstream_*
    section of include/gs_summary.h): per endpoint occurrence the row (vertex, old, new) with
    new = max(old + c, 0) -- SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees for
    direction "all" / "in" / "out" -- and the (degree, count) records example/DegreeDistribution.java
    emits at every change, exactly in arrival order however the stream is cut into folds.
    `reset`: no vertex, every count 0; capacity is kept. Owns a gs_degstream handle."""

    _PREFIX = "gs_degstream"

    DIRECTIONS = {"all": DEGREE_ALL, "in": DEGREE_IN, "out": DEGREE_OUT}

    def __init__(self, direction="all", device=0, vertex_hint=1 << 16):
        self.dir = self.DIRECTIONS[direction] if isinstance(direction, str) else int(direction)
        self.device = device
        h = _vp()
        _check(lib().gs_degstream_create(ctypes.byref(h), device, self.dir, int(vertex_hint)))
        self._h = h

    def fold(self, src, dst, deletions=None):
        """Fold host edges (int64 arrays) in order; deletions: optional uint8 per edge, bit 0 =
        deletion."""
        s, d = _edges(src, dst)
        e = None
        if deletions is not None:
            e = np.ascontiguousarray(np.asarray(deletions, dtype=np.uint8))
            assert e.shape == s.shape
        _check(lib().gs_degstream_fold(self._h, s.ctypes.data, d.ctypes.data, _ptr(e), len(s)))

    def fold_device(self, src, dst, n=None, stride=1, deletions=None, after=None):
        """Fold device-resident edges (torch tensors on this device or raw pointers), element i at
        index i * stride, deletions[i] its deletion byte; `after`: a stream the arrays were written
        on. The fold synchronises with the host once."""
        if n is None:
            n = (src.numel() + stride - 1) // stride
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_degstream_fold_device(self._h, _ptr(src), _ptr(dst), _ptr(deletions), int(n), int(stride)))

    def size(self):
        """gs_degstream_size. No device call."""
        out = (_u64 * 5)()
        _check(lib().gs_degstream_size(self._h, out))
        return {"vertices": out[0], "occurrences": out[1], "records": out[2], "total": out[3], "max_degree": out[4]}

    def rows(self):
        """The last fold's degree rows as numpy arrays (vertex int64, old uint32, new uint32), one
        per endpoint occurrence in arrival order."""
        got = _sz()
        n = max(self.size()["occurrences"], 1)
        v = np.empty(n, np.int64)
        o, w = (np.empty(n, np.uint32) for _ in range(2))
        _check(lib().gs_degstream_rows(self._h, v.ctypes.data, o.ctypes.data, w.ctypes.data, n, ctypes.byref(got)))
        k = got.value
        return v[:k].copy(), o[:k].copy(), w[:k].copy()

    def rows_device(self, vertex, old, new):
        """The same rows into DEVICE arrays (capacity of the first one given; any may be None);
        returns the row count."""
        got = _sz()
        _check(lib().gs_degstream_rows_device(self._h, _ptr(vertex), _ptr(old), _ptr(new), _cap_of(None, vertex, old, new),
                                              ctypes.byref(got)))
        return got.value

    def records(self):
        """The last fold's distribution records as numpy uint32 arrays (occurrence index in the
        fold, degree, count after the record), in arrival order."""
        got = _sz()
        n = max(self.size()["records"], 1)
        o, d, c = (np.empty(n, np.uint32) for _ in range(3))
        _check(lib().gs_degstream_records(self._h, o.ctypes.data, d.ctypes.data, c.ctypes.data, n, ctypes.byref(got)))
        k = got.value
        return o[:k].copy(), d[:k].copy(), c[:k].copy()

    def records_device(self, occurrence, degree, count):
        """The same records into DEVICE uint32 arrays; returns the record count."""
        got = _sz()
        _check(lib().gs_degstream_records_device(self._h, _ptr(occurrence), _ptr(degree), _ptr(count),
                                                 _cap_of(None, occurrence, degree, count), ctypes.byref(got)))
        return got.value

    def _state(self, name, sort):
        got = _sz()
        rc = getattr(lib(), name)(self._h, None, None, 0, ctypes.byref(got))
        if rc != GS_ERR_TRUNCATED:  # (the row count of a state with rows)
            _check(rc)
        n = max(got.value, 1)
        a, b = (np.empty(n, np.int64) for _ in range(2))
        _check(getattr(lib(), name)(self._h, a.ctypes.data, b.ctypes.data, n, ctypes.byref(got)))
        a, b = a[:got.value].copy(), b[:got.value].copy()
        if sort:
            order = np.argsort(a, kind="stable")
            a, b = a[order], b[order]
        return a, b

    def degrees(self, sorted=True):
        """(vertex, degree) numpy int64 arrays of the vertices with degree > 0: ascending by vertex
        (sorted on the host), or in first-seen order."""
        return self._state("gs_degstream_degrees", sorted)

    def degrees_device(self, vertex, degree):
        """The same rows, in first-seen order, into DEVICE int64 arrays; returns the row count."""
        got = _sz()
        _check(lib().gs_degstream_degrees_device(self._h, _ptr(vertex), _ptr(degree), _cap_of(None, vertex, degree),
                                                 ctypes.byref(got)))
        return got.value

    def distribution(self):
        """(degree, count) numpy int64 arrays: the degrees with count > 0, ascending."""
        return self._state("gs_degstream_distribution", False)

    def distribution_device(self, degree, count):
        """The distribution into DEVICE int64 arrays; returns its length."""
        got = _sz()
        _check(lib().gs_degstream_distribution_device(self._h, _ptr(degree), _ptr(count), _cap_of(None, degree, count),
                                                      ctypes.byref(got)))
        return got.value

    def stats(self):
        """gs_testing_degstream_stats: the last fold (synchronises)."""
        return self.phases()[0]

    def phases(self):
        """(stats, microseconds of the last fold's ranks and keys, sort by rank, clamped scan with
        the record counts and the control read, record rows with the sort by degree, seeded sum):
        the times are zero unless tune(profile=True)."""
        out = (_u64 * 9)()
        _check(lib().gs_testing_degstream_stats(self._h, out))
        return ({"tiles": out[0], "crossed": out[1], "count_capacity": out[2], "count_growths": out[3]},
                {"ranks": out[4], "sort_rank": out[5], "scan": out[6], "sort_degree": out[7], "sum": out[8]})

    def tune(self, profile=None):
        """gs_testing_degstream_tune, per handle: whether a fold times its phases (and then waits
        for the handle's stream a second time). None leaves the control as it is."""
        if profile is not None:
            _check(lib().gs_testing_degstream_tune(self._h, 0, 1 if profile else -1))


# ---------------------------------------------------------------- triangle streams
class TriangleStream(_ResetHandle):
    """Every record of example/ExactTriangleCount.java's continuous stream (the gs_tristream_*
    section of include/gs_summary.h): per arrival that closes c > 0 triangles the records
    (w, t(w) += 1) for every common neighbour w ascending, then (u, t(u) += c), (v, t(v) += c),
    and the row (closed, total); exactly in arrival order however the stream is cut into folds.
    repeats="count" (the reference) intersects a repeated pair again, "ignore" gives it c = 0.
    `reset`: G empty, every counter 0; capacity is kept. Owns a gs_tristream handle."""

    _PREFIX = "gs_tristream"

    def __init__(self, repeats="count", edge_hint=0, device=0):
        self.repeats = TRISTREAM_REPEATS[repeats] if isinstance(repeats, str) else int(repeats)
        self.device = device
        h = _vp()
        _check(lib().gs_tristream_create(ctypes.byref(h), device, self.repeats, int(edge_hint)))
        self._h = h

    def fold(self, src, dst):
        """Fold host arrivals (int64 arrays) in order."""
        s, d = _edges(src, dst)
        _check(lib().gs_tristream_fold(self._h, s.ctypes.data, d.ctypes.data, len(s)))

    def fold_device(self, src, dst, n=None, stride=1, after=None):
        """Fold device-resident arrivals (torch tensors on this device or raw pointers), element i
        at index i * stride; `after`: a stream the arrays were written on. The fold synchronises
        with the host twice."""
        if n is None:
            n = (src.numel() + stride - 1) // stride
        if after is not None:
            self.wait_stream(after)
        _check(lib().gs_tristream_fold_device(self._h, _ptr(src), _ptr(dst), int(n), int(stride)))

    def size(self):
        """gs_tristream_size. No device call."""
        out = (_u64 * 4)()
        _check(lib().gs_tristream_size(self._h, out))
        return {"arrivals": out[0], "records": out[1], "new_pairs": out[2], "total": out[3]}

    def count(self):
        """gs_tristream_count: T, |G|, the vertices of G, the arrivals since reset (synchronises)."""
        out = (_u64 * 4)()
        _check(lib().gs_tristream_count(self._h, out))
        return {"triangles": out[0], "edges": out[1], "vertices": out[2], "arrivals": out[3]}

    def rows(self):
        """The last fold's rows as numpy arrays (closed uint32, total int64), one per arrival."""
        got = _sz()
        n = max(self.size()["arrivals"], 1)
        c = np.empty(n, np.uint32)
        t = np.empty(n, np.int64)
        _check(lib().gs_tristream_rows(self._h, c.ctypes.data, t.ctypes.data, n, ctypes.byref(got)))
        k = got.value
        return c[:k].copy(), t[:k].copy()

    def rows_device(self, closed, total):
        """The same rows into DEVICE arrays (capacity of the first one given; either may be None);
        returns the row count."""
        got = _sz()
        _check(lib().gs_tristream_rows_device(self._h, _ptr(closed), _ptr(total), _cap_of(None, closed, total),
                                              ctypes.byref(got)))
        return got.value

    def records(self):
        """The last fold's records as numpy arrays (arrival index in the fold uint32, vertex int64,
        count int64), in emission order."""
        got = _sz()
        n = max(self.size()["records"], 1)
        a = np.empty(n, np.uint32)
        v, c = (np.empty(n, np.int64) for _ in range(2))
        _check(lib().gs_tristream_records(self._h, a.ctypes.data, v.ctypes.data, c.ctypes.data, n, ctypes.byref(got)))
        k = got.value
        return a[:k].copy(), v[:k].copy(), c[:k].copy()

    def records_device(self, arrival, vertex, count):
        """The same records into DEVICE arrays; returns the record count."""
        got = _sz()
        _check(lib().gs_tristream_records_device(self._h, _ptr(arrival), _ptr(vertex), _ptr(count),
                                                 _cap_of(None, arrival, vertex, count), ctypes.byref(got)))
        return got.value

    def local_counts(self):
        """(vertex, t) numpy int64 arrays of the vertices with t > 0, ascending by vertex."""
        got = _sz()
        rc = lib().gs_tristream_counts(self._h, None, None, 0, ctypes.byref(got))
        if rc != GS_ERR_TRUNCATED:  # (the row count of a state with rows)
            _check(rc)
        n = max(got.value, 1)
        v, c = (np.empty(n, np.int64) for _ in range(2))
        _check(lib().gs_tristream_counts(self._h, v.ctypes.data, c.ctypes.data, n, ctypes.byref(got)))
        return v[:got.value].copy(), c[:got.value].copy()

    def local_counts_device(self, vertex, count):
        """The same rows into DEVICE int64 arrays; returns the row count."""
        got = _sz()
        _check(lib().gs_tristream_counts_device(self._h, _ptr(vertex), _ptr(count), _cap_of(None, vertex, count),
                                                ctypes.byref(got)))
        return got.value

    def stats(self):
        """gs_testing_tristream_stats: the last fold (synchronises)."""
        return self.phases()[0]

    def phases(self):
        """(stats, microseconds of the last fold's ranks with sort and dedupe, merge, rows and count,
        offsets and write, record ranks and sort, scan and counters): the times are zero unless
        tune(profile=True)."""
        out = (_u64 * 10)()
        _check(lib().gs_testing_tristream_stats(self._h, out))
        return ({"tiles": out[0], "crossed": out[1], "longest_row": out[2], "steps": out[3]},
                {"sort_dedupe": out[4], "merge": out[5], "count": out[6], "write": out[7], "record_sort": out[8],
                 "scan": out[9]})

    def tune(self, profile=None, max_records=None):
        """gs_testing_tristream_tune, per handle: whether a fold times its phases (and then waits
        for the handle's stream once more), and the records a fold may emit before it fails with
        GS_ERR_CAPACITY (a value <= 0 restores TRISTREAM_MAX_RECORDS). None leaves a control as it
        is."""
        if profile is not None:
            _check(lib().gs_testing_tristream_tune(self._h, 0, 1 if profile else -1))
        if max_records is not None:
            _check(lib().gs_testing_tristream_tune(self._h, 1, int(max_records)))


# ---------------------------------------------------------------- native multi-GPU group
GROUP_ID_BYTES = 256  # two RCCL unique ids (count and data communicators)


def group_unique_id():
    """RCCL communicator id (bytes) for Group(); create on one rank, share with all."""
    buf = ctypes.create_string_buffer(GROUP_ID_BYTES)
    _check(lib().gs_group_unique_id(buf))
    return buf.raw


class Group:
    """Native multi-GPU combine (include/gs_group.h): per global micro-batch,
    fold this rank's edges, all-gather the delta counts and then exactly the live
    records over RCCL, fold the other ranks' records. Collective calls."""

    def __init__(self, summary, uid, nranks, rank, batch_edges):
        g = _vp()
        buf = ctypes.create_string_buffer(bytes(uid), GROUP_ID_BYTES)
        _check(lib().gs_group_create(ctypes.byref(g), summary.handle, buf, int(nranks), int(rank),
                                     int(batch_edges)))
        self._g = g
        self.summary = summary

    def fold_device(self, src, dst, n):
        _check(lib().gs_group_fold_device(self._g, _ptr(src), _ptr(dst), int(n)))

    def fold_batches(self, src, dst, n, batch):
        """ceil(n / batch) micro-batches of fold_device, looped in native code."""
        _check(lib().gs_group_fold_batches_device(self._g, _ptr(src), _ptr(dst), int(n), int(batch)))

    def set_ramp(self, edges, batch=1 << 20):
        """fold_batches exchanges the first `edges` own edges after create / finish every
        `batch` edges (gs_group_set_ramp; 0 disables). Same on every rank."""
        _check(lib().gs_group_set_ramp(self._g, int(edges), int(batch)))

    def finish(self):
        _check(lib().gs_group_finish(self._g))

    def tree_combine(self):
        """Binomial-tree combine of per-rank partial summaries onto rank 0
        (gs_group_tree_combine; SummaryTreeReduce). Collective, synchronous."""
        _check(lib().gs_group_tree_combine(self._g))

    def stats(self):
        e, s, c = _u64(), _u64(), _u64()
        _check(lib().gs_group_stats(self._g, ctypes.byref(e), ctypes.byref(s), ctypes.byref(c)))
        return {"exchanges": e.value, "records_sent": s.value, "rows_received": c.value}

    def comm_ranks(self):
        """(ranks of the count communicator, ranks of the data communicator): ncclCommCount."""
        c, d = ctypes.c_int(), ctypes.c_int()
        _check(lib().gs_group_comm_ranks(self._g, ctypes.byref(c), ctypes.byref(d)))
        return c.value, d.value

    def set_phase_timing(self, on=True):
        _check(lib().gs_group_set_phase_timing(self._g, 1 if on else 0))

    def phase_stats(self):
        """Per-phase device milliseconds since set_phase_timing (gs_group_phase_stats)."""
        out = (ctypes.c_double * 6)()
        _check(lib().gs_group_phase_stats(self._g, out))
        return {"own_fold_lane_ms": out[0], "remote_fold_ms": out[1], "stage_count_collective_ms": out[2],
                "data_collective_ms": out[3], "host_wait_counts_ms": out[4], "exchanges": int(out[5])}

    def close(self):
        if getattr(self, "_g", None):
            lib().gs_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PartGroup:
    """Owner-partitioned multi-GPU combine (include/gs_group.h gs_group_create_partitioned;
    DESIGN.md section 5b): each rank folds its own edges into a LOCAL forest (`summary`),
    and every combine sends the new local labels to the vertices' owners, which keep one
    anchor per vertex and feed the label pairs to every rank's label forest. labels()
    returns this rank's owned slice. Collective calls: create, combine."""

    def __init__(self, summary, uid, nranks, rank, vertices_hint, window_edges=0):
        g = _vp()
        buf = ctypes.create_string_buffer(bytes(uid), GROUP_ID_BYTES)
        _check(lib().gs_group_create_partitioned(ctypes.byref(g), summary.handle, buf, int(nranks), int(rank),
                                                 int(vertices_hint), int(window_edges)))
        self._g = g
        self.summary = summary

    def fold_device(self, src, dst, n):
        _check(lib().gs_group_part_fold_device(self._g, _ptr(src), _ptr(dst), int(n)))

    def combine(self):
        _check(lib().gs_group_part_combine(self._g))

    def labels_device(self, v, label, parity=None):
        got = _sz()
        cap = v.numel() if hasattr(v, "numel") else len(v)
        _check(lib().gs_group_part_labels_device(self._g, _ptr(v), _ptr(label), _ptr(parity), int(cap),
                                                 ctypes.byref(got)))
        return got.value

    def labels(self, cap, with_parity=False):
        """This rank's owned (v, label[, parity]) as numpy arrays sorted by v."""
        import torch
        dev = torch.device("cuda", self.summary.device)
        v = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        lab = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        par = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev) if with_parity else None
        k = self.labels_device(v, lab, par)
        hv, hl = v[:k].cpu().numpy(), lab[:k].cpu().numpy()
        o = np.argsort(hv, kind="stable")
        if with_parity:
            return hv[o], hl[o], par[:k].cpu().numpy()[o]
        return hv[o], hl[o]

    def ok(self):
        o = ctypes.c_int()
        _check(lib().gs_group_part_status(self._g, ctypes.byref(o)))
        return bool(o.value)

    def comm_ranks(self):
        """(ranks of the count communicator, ranks of the data communicator): ncclCommCount."""
        c, d = ctypes.c_int(), ctypes.c_int()
        _check(lib().gs_group_comm_ranks(self._g, ctypes.byref(c), ctypes.byref(d)))
        return c.value, d.value

    def reset(self):
        _check(lib().gs_group_part_reset(self._g))

    def stats(self):
        a = (_u64 * 8)()
        _check(lib().gs_group_part_stats(self._g, a))
        keys = ("combines", "rows_exported", "rows_owned", "pairs_sent", "pairs_folded", "label_forest_vertices",
                "owner_slots")
        return dict(zip(keys, list(a)))

    def set_phase_timing(self, on=True):
        _check(lib().gs_group_set_phase_timing(self._g, 1 if on else 0))

    def forest_counters(self):
        """Diagnostics of the label forest (include/gs_testing.h gs_testing_group_forest):
        gs_counters (vertices, hooks, hook-loop iterations, failed hook CASes -- the last three
        in the debug build) and gs_debug_counters (debug build, GS_LIB_VARIANT=debug)."""
        f = _vp()
        _check(lib().gs_testing_group_forest(self._g, ctypes.byref(f)))
        a, d = (_u64 * 8)(), (_u64 * 16)()
        _check(lib().gs_counters(f, a))
        _check(lib().gs_debug_counters(f, d, 16))
        out = dict(zip(("vertices", "failed", "err", "ovf", "sent", "hooks", "hook_iters", "cas_fail"), list(a)))
        out.update(zip(("edges", "key_cas", "key_cas_lost", "ttas", "shortcut", "same_root", "find_loads", "hooks_ok",
                        "extra_probes"), list(d)))
        return out

    def phase_stats(self):
        out = (ctypes.c_double * 8)()
        _check(lib().gs_group_part_phase_stats(self._g, out))
        keys = ("own_fold_ms", "export_ms", "bucket_ms", "alltoall_ms", "owner_ms", "pair_gather_ms", "forest_fold_ms",
                "combines")
        return dict(zip(keys, list(out)))

    def close(self):
        if getattr(self, "_g", None):
            lib().gs_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- generators
def parse_edges_device(text, src, dst, sep=SEP_WHITESPACE, stream=None):
    """gs_parse_edges_device: device uint8 text -> device int64 src/dst. Returns
    (n_lines, bad_line); bad_line = first malformed line or -1 (no exception for a
    malformed line or a short output: the caller compares n_lines with capacity)."""
    n = _u64()
    bad = _i64(-1)
    ln = text.numel() if hasattr(text, "numel") else len(text)
    cap = src.numel() if hasattr(src, "numel") else len(src)
    rc = lib().gs_parse_edges_device(stream, _ptr(text), ln, int(sep), _ptr(src), _ptr(dst), cap, ctypes.byref(n),
                                     ctypes.byref(bad))
    if rc not in (GS_OK, GS_ERR_PARSE, GS_ERR_TRUNCATED):
        raise GSError(rc, "gs_parse_edges_device failed")
    return n.value, bad.value


def _text_flags(int32, comments):
    return (TEXT_INT32 if int32 else 0) | (TEXT_COMMENT_PERCENT if comments else 0)


def parse_records_device(text, src, dst, third_out=None, sep=SEP_WHITESPACE, third=None, int32=False, comments=False,
                         stream=None):
    """gs_parse_records_device: device uint8 text -> device int64 src/dst and, for third "long" /
    "event", the int64 values / uint8 deletion bytes in `third_out`. The capacity counts lines.
    Returns (n_lines, n_records, bad_line); as parse_edges_device, a malformed line or a short
    output raises nothing."""
    if third not in TEXT_THIRD:
        raise ValueError("third must be None, 'long' or 'event'")
    nl, nr, bad = _u64(), _u64(), _i64(-1)
    ln = text.numel() if hasattr(text, "numel") else len(text)
    cap = src.numel() if hasattr(src, "numel") else len(src)
    val = _ptr(third_out) if third == "long" else None
    dele = _ptr(third_out) if third == "event" else None
    rc = lib().gs_parse_records_device(stream, _ptr(text), ln, int(sep), TEXT_THIRD[third], _text_flags(int32, comments),
                                       _ptr(src), _ptr(dst), val, dele, cap, ctypes.byref(nl), ctypes.byref(nr),
                                       ctypes.byref(bad))
    if rc not in (GS_OK, GS_ERR_PARSE, GS_ERR_TRUNCATED):
        raise GSError(rc, "gs_parse_records_device failed")
    return nl.value, nr.value, bad.value


def window_bounds_device(ts, size, first, window, n=None, stream=None):
    """gs_window_bounds_device: the event-time windows (id = ts / size, truncating) of the device
    int64 timestamps ts[:n]: first[w] (uint64 as int64 tensor) and window[w] for every maximal run
    of equal ids. Returns the number of windows (it may exceed the capacity of first / window)."""
    nw = _u64()
    if n is None:
        n = ts.numel()
    cap = min(first.numel(), window.numel())
    rc = lib().gs_window_bounds_device(stream, _ptr(ts), int(n), int(size), _ptr(first), _ptr(window), cap,
                                       ctypes.byref(nw))
    if rc not in (GS_OK, GS_ERR_TRUNCATED):
        raise GSError(rc, "gs_window_bounds_device failed")
    return nw.value


def testing_text_stats():
    """gs_testing_text_stats: (field-spec parses, comment compactions) of parse_records_device."""
    out = (_u64 * 2)()
    _check(lib().gs_testing_text_stats(out))
    return out[0], out[1]


class _DeviceColumn:
    """n elements of device memory at ptr, for torch.as_tensor (the CUDA array interface)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


def _device_view(ptr, n, typestr, device):
    import torch
    dtype = {"<i8": torch.int64, "|u1": torch.uint8}[typestr]
    if not ptr or n == 0:
        return torch.empty(0, dtype=dtype, device="cuda:%d" % device)
    return torch.as_tensor(_DeviceColumn(ptr, n, typestr), device="cuda:%d" % device)


class TextReader(_Handle):
    """A gs_text reader: host text (bytes) in, chunks of device columns out, for any handle's
    fold_device. third: None, "long" (a Long.parseLong value or timestamp) or "event" ('+' /
    anything else: the deletion byte); int32: Integer.parseInt endpoints; comments: "%" lines
    give no record (include/gs_ingest.h states the rules). The tensors a chunk yields are views
    of the reader's columns: they hold until the chunk after the next is asked for."""

    _PREFIX = "gs_text"

    def __init__(self, device=0, sep=SEP_WHITESPACE, third=None, int32=False, comments=False, chunk_bytes=0):
        if third not in TEXT_THIRD:
            raise ValueError("third must be None, 'long' or 'event'")
        self._h = None
        self.device = device
        self.third = third
        self.sep = sep
        h = _vp()
        _check(lib().gs_text_create(ctypes.byref(h), device, int(sep), TEXT_THIRD[third], _text_flags(int32, comments),
                                    int(chunk_bytes)))
        self._h = h

    def position(self):
        """(lines, records, bad_line) since the last open; bad_line -1 unless a malformed line ended it."""
        nl, nr, bad = _u64(), _u64(), _i64(-1)
        self._call("position", ctypes.byref(nl), ctypes.byref(nr), ctypes.byref(bad))
        return nl.value, nr.value, bad.value

    def _next(self):
        p = [_vp() for _ in range(6)]
        n, nw, last = _sz(), _sz(), ctypes.c_int()
        self._call("next", ctypes.byref(p[0]), ctypes.byref(p[1]), ctypes.byref(p[2]), ctypes.byref(p[3]),
                   ctypes.byref(n), ctypes.byref(p[4]), ctypes.byref(p[5]), ctypes.byref(nw), ctypes.byref(last))
        return [x.value for x in p], n.value, nw.value, bool(last.value)

    def _chunks(self, text, window):
        text = bytes(text)  # (kept alive until the last chunk)
        self._call("set_window", int(window))
        self._call("open", text, len(text))
        last = False
        while not last:
            p, n, nw, last = self._next()
            src = _device_view(p[0], n, "<i8", self.device)
            dst = _device_view(p[1], n, "<i8", self.device)
            third = None
            if self.third == "long":
                third = _device_view(p[2], n, "<i8", self.device)
            elif self.third == "event":
                third = _device_view(p[3], n, "|u1", self.device)
            yield src, dst, third, n, _device_view(p[4], nw, "<i8", self.device), _device_view(p[5], nw, "<i8",
                                                                                               self.device)

    def chunks(self, text):
        """A generator of (src, dst, third, n): the records of one chunk as device tensors (third:
        int64 values, uint8 deletion bytes, or None). The chunk is complete on the reader's stream
        and the host has waited for it. A malformed line raises GSError(GS_ERR_PARSE) when its chunk
        is reached; position() then names its line."""
        for src, dst, third, n, _, _ in self._chunks(text, 0):
            yield src, dst, third, n

    def windows(self, text, size):
        """A generator of (window_id, src, dst, val, n), one per whole event-time window (third
        "long": the timestamps; id = ts / size, truncating), in stream order."""
        if self.third != "long":
            raise ValueError("windows need a reader with third='long' (the timestamp)")
        if int(size) <= 0:
            raise ValueError("a window size is > 0")
        for src, dst, val, n, first, window in self._chunks(text, int(size)):
            f = first.cpu().tolist() + [n]
            for k, w in enumerate(window.cpu().tolist()):
                a, b = f[k], f[k + 1]
                yield w, src[a:b], dst[a:b], val[a:b], b - a

    def _fold_kind(self, target):
        """How fold_into hands a chunk to `target`: "plain", "deletions" or "val"; ValueError for a
        target this reader's third field does not fit."""
        name = type(target).__name__
        if isinstance(target, (Degrees, DegreeStream)):
            if self.third == "long":
                raise ValueError("%s takes an 'event' reader (deletions) or one without a third field" % name)
            return "deletions" if self.third == "event" else "plain"
        if isinstance(target, Matching):
            if self.third != "long":
                raise ValueError("Matching needs a reader with third='long' (the weight)")
            return "val"
        if isinstance(target, (Summary, Triangles, TriangleStream, Distinct, Spanner, TriangleSampler)):
            if self.third is not None:
                raise ValueError("%s takes a reader without a third field" % name)
            return "plain"
        raise ValueError("fold_into: no fold for a %s" % name)

    def fold_into(self, target, text, each=None):
        """Fold every chunk of `text` into `target` with its fold_device, in order; each(n), if
        given, runs after each chunk's fold (a stream handle's rows can be read there). The
        target's stream waits for the reader's before a fold, and the reader's for the target's
        before the next chunk overwrites columns a fold may still read. Returns the record count.
        Degrees / DegreeStream take an "event" reader (deletions) or one without a third field,
        Matching a "long" one (the weight), every other handle one without a third field; a
        mismatch raises ValueError before anything is folded."""
        kind = self._fold_kind(target)
        total = 0
        own = self.stream
        for src, dst, third, n in self.chunks(text):
            if n:
                target.wait_stream(own)
                if kind == "deletions":
                    target.fold_device(src, dst, n=n, deletions=third)
                elif kind == "val":
                    target.fold_device(src, dst, third, n=n)
                else:
                    target.fold_device(src, dst, n=n)
                self.wait_stream(target.stream)
            total += n
            if each is not None:
                each(n)
        return total


def parse_set_profiling(on):
    """gs_parse_set_profiling: time each parse kernel of this thread with HIP events."""
    rc = lib().gs_parse_set_profiling(1 if on else 0)
    if rc:
        raise GSError(rc, "gs_parse_set_profiling failed")


def parse_profile():
    """gs_parse_profile: (summed parse-kernel microseconds, parses) since profiling was turned on."""
    us = ctypes.c_double()
    n = _u64()
    rc = lib().gs_parse_profile(ctypes.byref(us), ctypes.byref(n))
    if rc:
        raise GSError(rc, "gs_parse_profile failed")
    return us.value, n.value


def parse_release():
    """gs_parse_release: free this thread's parse cache (device scratch, mapped record, events)."""
    rc = lib().gs_parse_release()
    if rc:
        raise GSError(rc, "gs_parse_release failed")


def gen_rmat(src, dst, start, count, scale, seed, scramble=True, stream=None):
    rc = lib().gs_gen_rmat(stream, _ptr(src), _ptr(dst), start, count, scale, seed, 1 if scramble else 0)
    if rc:
        raise GSError(rc, "gs_gen_rmat failed")


def gen_er(src, dst, start, count, logn, seed, scramble=True, stream=None):
    rc = lib().gs_gen_er(stream, _ptr(src), _ptr(dst), start, count, logn, seed, 1 if scramble else 0)
    if rc:
        raise GSError(rc, "gs_gen_er failed")


def gen_bip(src, dst, start, count, logside, seed, inject=(), stream=None):
    inj = np.ascontiguousarray(np.sort(np.asarray(inject, dtype=np.uint64)))
    rc = lib().gs_gen_bip(stream, _ptr(src), _ptr(dst), start, count, logside, seed,
                          inj.ctypes.data if len(inj) else None, len(inj))
    if rc:
        raise GSError(rc, "gs_gen_bip failed")


def relabel_first_appearance(src, dst, id_bound):
    """Rename the vertices of a device edge stream (torch int64 tensors, ids in
    [0, id_bound)) in place to 1, 2, 3, ... in order of first appearance (edge by edge,
    src before dst): SURVEY.md 8(d) config 4's ids, the reference's exact regime
    (with such ids and one window, Candidates.merge -- Candidates.java:
    77-192 -- returns the canonical colouring). A renaming is a graph isomorphism, so
    verdicts and the window where one flips are unchanged. Stream preparation (bench and
    tests), outside any timed region; torch ops on the current stream."""
    import torch
    n = src.numel()
    occ = torch.stack([src, dst], 1).reshape(-1)  # occurrence order: s0, d0, s1, d1, ...
    pos = torch.arange(2 * n, dtype=torch.int64, device=src.device)
    first = torch.full((id_bound,), 2 * n, dtype=torch.int64, device=src.device)
    first.scatter_reduce_(0, occ, pos, reduce="amin")
    del pos
    flag = torch.zeros(2 * n + 1, dtype=torch.int64, device=src.device)
    flag[first] = 1  # first occurrence of every vertex (unseen ids mark the sentinel slot 2n)
    rank = torch.cumsum(flag[:2 * n], 0)  # 1-based rank of each first occurrence
    new = rank[first[occ]]
    src.copy_(new[0::2])
    dst.copy_(new[1::2])
