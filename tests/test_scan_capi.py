"""CPU: the flag / scan / compact idiom has one copy. The wave scan is defined in gs_scan.hpp
alone, the four kernel files that compact include it and call its workgroup primitives, and the
one tile-count scan the headers declare is gs_sort.hpp's launch_tile_scan. No compute calls here
(the results are checked on the GPU in test_gpu_slice.py, test_gpu_distinct.py,
test_gpu_triangles.py and test_gpu_components.py)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gelly-streaming_amd", "csrc")
USERS = ("gs_sort_k.hip", "gs_slice_k.hip", "gs_distinct_k.hip", "gs_triangle_k.hip")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_wave_scan_is_defined_once():
    defined = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*")))
               if re.search(r"\bwave_incl_scan\(uint32_t \w+\) \{", _read(p))]
    assert defined == ["gs_scan.hpp"]
    text = _read("gs_scan.hpp")
    for fn in ("uint32_t block_excl_scan(uint32_t cnt, uint32_t* wsum)",
               "void block_count_to(uint32_t cnt, uint32_t* total_lds, uint32_t* out)"):
        assert fn in text, fn
    assert "__global__" not in text  # device functions only: no kernel per including code object


def test_kernels_include_the_shared_header():
    for name in USERS:
        text = _read(name)
        assert '#include "gs_scan.hpp"' in text, name
        for fn in ("block_excl_scan<", "block_count_to<"):
            assert fn in text, (name, fn)
        # none sums the earlier waves' counts itself again
        assert not re.search(r"if \(q < wid\) \w+ \+= ", text), name
    with open(os.path.join(ROOT, "gelly-streaming_amd", "Makefile")) as f:
        assert "csrc/gs_scan.hpp" in re.search(r"^HDRS := (.*)$", f.read(), re.M).group(1)


def test_one_tile_count_scan_is_declared():
    scans = []
    for p in sorted(glob.glob(os.path.join(CSRC, "*.hpp"))):
        scans += [(os.path.basename(p), m) for m in re.findall(r"\bvoid (launch_\w*scan\w*)\(", _read(p))]
    # (the other two are no tile-count scans: the change emission's scan of the whole table, and the
    # partitioned group's per-owner offsets of its export blocks)
    assert scans == [("gs_kernels.hpp", "launch_emit_scan"), ("gs_part.hpp", "launch_part_scan"),
                     ("gs_sort.hpp", "launch_tile_scan")]
    assert "uint32_t* tb, uint64_t nt, unsigned long long* total, hipStream_t st" in _read("gs_sort.hpp")
    for name in ("gs_slice_k.hip", "gs_distinct_k.hip", "gs_triangle.cpp"):
        assert "launch_tile_scan(" in _read(name), name
    for name in USERS:  # and the scan kernels by their names: k_sort_scan scans digit rows, k_tile_scan tile counts
        kernels = re.findall(r"void (k_\w*scan\w*)\(", _read(name))
        assert kernels == (["k_sort_scan", "k_tile_scan"] if name == "gs_sort_k.hip" else []), name
