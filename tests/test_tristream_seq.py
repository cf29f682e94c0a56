"""CPU: the triangle streams' rules header (csrc/gs_tristream_seq.hpp: the stamp test, the record
layout, the segmented combine, the sequential definition trs_fold_seq and the kernels'
decomposition trs_fold_parts) in a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/cpp/tristream_seq_sanitize.cpp): trs_fold_seq against a
literal restatement of the reference's three operators, trs_fold_parts against trs_fold_seq at every
tile size and every cut, and the pins of tests/golden/tristream_pins.json. The header is the one
the kernels include."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gelly-streaming_amd", "csrc")


def _pins():
    with open(os.path.join(ROOT, "tests", "golden", "tristream_pins.json")) as f:
        return json.load(f)


def _pins_text():
    """The pins as the program reads them: '#name count' and then count lines of integers."""
    pins = _pins()
    sections = {}
    for k, case in enumerate(pins["test_intersection"]["cases"]):
        sections["stream_%d" % k] = case["as_stream"]
        sections["records_%d" % k] = case["stream_records"]
        sections["total_%d" % k] = [[case["stream_total"]]]
        sections["tuples_%d" % k] = case["expected_tuples"]
    sections["builtin"] = pins["builtin_stream"]["edges"]
    sections["derived_tuples"] = pins["derived"]["tuples"]
    sections["derived_rows"] = [list(r) for r in zip(pins["derived"]["closed"], pins["derived"]["totals"])]
    sections["counts_in"] = pins["test_counts"]["inputs"]
    sections["counts_out"] = pins["test_counts"]["running_sums"]
    return "".join("#%s %d\n%s\n" % (k, len(v), "\n".join(" ".join(str(x) for x in row) for row in v))
                   for k, v in sections.items())


def test_pins_are_consistent():
    pins = _pins()
    for case in pins["test_intersection"]["cases"]:
        # the restated stream gives the endpoints exactly the pinned neighbourhoods at the last arrival
        u, v = case["key"]
        hood = {}
        for s, d in case["as_stream"]:
            hood.setdefault(s, set()).add(d)
            hood.setdefault(d, set()).add(s)
        assert case["as_stream"][-1] == [u, v]
        assert sorted(hood[u]) == case["first_neighborhood"] and sorted(hood[v]) == case["second_neighborhood"]
        assert case["stream_records"] + [[-1, case["stream_total"]]] == case["expected_tuples"]
    d = pins["derived"]
    assert len(d["closed"]) == len(d["totals"]) == len(pins["builtin_stream"]["edges"]) == 9
    flat = []
    for a in range(9):
        flat += [[v, c] for i, v, c in d["records"] if i == a]
        if d["closed"][a]:
            flat.append([-1, d["totals"][a]])
    assert flat == d["tuples"]
    assert "ExactTriangleCount.java:196-205" in pins["builtin_stream"]["source"]
    assert "not recorded output" in d["source"]


def test_rules_and_decomposition_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "tristream_seq_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + CSRC,
                            os.path.join(ROOT, "tests", "cpp", "tristream_seq_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    pins = tmp_path / "pins.txt"
    pins.write_text(_pins_text())
    # a preloaded library may precede the ASan runtime: do not treat that as an error
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(pins)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_kernels_and_host_include_the_checked_header():
    with open(os.path.join(CSRC, "gs_tristream.hpp")) as f:
        hpp = f.read()
    assert '#include "gs_tristream_seq.hpp"' in hpp and '#include "gs_distinct.hpp"' in hpp
    with open(os.path.join(CSRC, "gs_tristream_k.hip")) as f:
        text = f.read()
    assert '#include "gs_tristream.hpp"' in text and '#include "gs_scan.hpp"' in text
    assert '#include "gs_triangle_rows.hpp"' in text
    for fn in ("trs_seg_combine(", "trs_seg_element(", "trs_seg_after(", "trs_seg_identity(", "trs_hit(", "trs_pick_rows(",
               "trs_arrival_no(", "trs_record_count(", "trs_record_delta(", "trs_tiles(", "tri_merge_pos(", "tri_row(",
               "block_excl_scan<", "block_count_to<", "__ballot(", "__popcll("):
        assert fn in text, fn
    with open(os.path.join(CSRC, "gs_tristream.cpp")) as f:
        host = f.read()
    assert '#include "gs_tristream.hpp"' in host and '#include "gs_vtable.hpp"' in host
    for fn in ("kTrsMaxTotal", "kTrsMaxFold", "kTrsMaxRecords", "launch_dist_vertices(", "launch_dist_rank(",
               "launch_tri_canon(", "launch_tri_flag_new(", "launch_tile_scan(", "sort_by_pair(", "sort_by_key(",
               "sort_skip_above(", "grow_group(", "check_handle(", "GS_LAUNCH(", ": StreamOwner, VertexTable"):
        assert fn in host, fn
    # the definition and the decomposition are made of the same rules
    with open(os.path.join(CSRC, "gs_tristream_seq.hpp")) as f:
        seq = f.read()
    for fn in ("trs_canon(", "trs_stamp_ok(", "trs_arrival_no(", "trs_record_count(", "trs_seg_combine(", "trs_hit("):
        assert seq.count(fn) >= 2, fn
    assert "inline void trs_fold_seq(" in seq and "inline uint64_t trs_fold_parts(" in seq
    # no second open-addressing insert, no inline assembly
    assert "atomicCAS" not in text and "atomicCAS" not in host and "asm" not in text
    # no workgroup waits on another: no spin, no grid-wide barrier
    assert "while (" not in text and "cooperative" not in text
    # the header reads standard headers and the row arithmetic only (and the HIP runtime under a HIP compiler)
    incs = [ln.split()[1] for ln in seq.splitlines() if ln.startswith("#include")]
    assert all(i.startswith("<") or i == '"gs_triangle_rows.hpp"' for i in incs), incs
