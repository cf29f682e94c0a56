"""CPU: the grouped component export's three entry points exist, are declared and bound,
and reject null arguments before touching a device. No compute calls here (the results
are checked on the GPU in test_gpu_components.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_num_components", "gs_export_components_device", "gs_export_components")


def test_exported_symbols_contain_the_three_names(gs):
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(gs.LIB_PATH), n)
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\bint %s\(gs_handle h," % n, text), n


def test_null_handle_is_rejected(gs):
    L = gs.lib()
    n = ctypes.c_uint64(7)
    nv, nc = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.gs_num_components(None, ctypes.byref(n)) == gs.GS_ERR_INVALID
    assert b"null" in L.gs_last_error()
    for fn in (L.gs_export_components_device, L.gs_export_components):
        assert fn(None, None, None, None, None, 0, 0, ctypes.byref(nv), ctypes.byref(nc)) == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()


def test_null_counts_are_rejected(gs):
    L = gs.lib()
    assert L.gs_num_components(None, None) == gs.GS_ERR_INVALID
    nv = ctypes.c_size_t(0)
    for fn in (L.gs_export_components_device, L.gs_export_components):
        assert fn(None, None, None, None, None, 0, 0, None, None) == gs.GS_ERR_INVALID
        assert fn(None, None, None, None, None, 0, 0, ctypes.byref(nv), None) == gs.GS_ERR_INVALID
        assert fn(None, None, None, None, None, 0, 0, None, ctypes.byref(nv)) == gs.GS_ERR_INVALID


def test_python_class_has_the_calls(gs):
    for m in ("num_components", "components_device", "components"):
        assert callable(getattr(gs.Summary, m))


def test_sort_tile_constant_matches_the_kernels(gs):
    """gsamd.SORT_TILE (the sizes test_gpu_components.py brackets) is kSortBS * kSortItems."""
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_sort.hpp")) as f:
        text = f.read()
    bs = int(re.search(r"kSortBS = (\d+);", text).group(1))
    items = int(re.search(r"kSortItems = (\d+);", text).group(1))
    assert gs.SORT_TILE == bs * items


def test_tile_scan_block_constant_matches_the_kernels(gs):
    """gsamd.TILE_SCAN_BLOCK (the step test_gpu_slice.py, test_gpu_distinct.py and
    test_gpu_triangles.py cross) is kSortScanBS, the workgroup of k_tile_scan."""
    csrc = os.path.join(ROOT, "gelly-streaming_amd", "csrc")
    with open(os.path.join(csrc, "gs_sort.hpp")) as f:
        assert gs.TILE_SCAN_BLOCK == int(re.search(r"kSortScanBS = (\d+);", f.read()).group(1))
    with open(os.path.join(csrc, "gs_sort_k.hip")) as f:
        text = f.read()
    assert re.search(r"__launch_bounds__\(kSortScanBS\) void k_tile_scan\(", text)
    assert re.search(r"hipLaunchKernelGGL\(k_tile_scan, dim3\(1\), dim3\(kSortScanBS\)", text)
    assert re.search(r"c0 < nt; c0 \+= kSortScanBS\)", text)
