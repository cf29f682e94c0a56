"""CPU: the distinct streams' stamp encodings, keep predicates, key packing, growth and tile
arithmetic (csrc/gs_distinct_seq.hpp) against brute force in a stand-alone program built with the
address and undefined-behaviour sanitizers (tests/cpp/distinct_seq_sanitize.cpp). The header is
the one the kernels include."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_walk_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "distinct_seq_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "gelly-streaming_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "distinct_seq_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    # a preloaded library may precede the ASan runtime: do not treat that as an error
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_kernels_include_the_checked_header():
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_distinct_k.hip")) as f:
        text = f.read()
    assert '#include "gs_distinct_seq.hpp"' in text
    for fn in ("dist_vertex_stamp(", "dist_vertex_skip(", "dist_vertex_keep(", "dist_edge_key(", "dist_key_ranks(",
               "dist_edge_stamp(", "dist_stamp_arrival(", "dist_stamp_swapped(", "dist_edge_old(", "dist_edge_skip(",
               "dist_edge_keep(", "dist_vertex_home(", "dist_edge_home(", "dist_entry_edge(", "dist_entry_is_dst(",
               "dist_tiles(", "dist_flag_pos(", "dist_write_first(", "dist_out_row("):
        assert fn in text, fn
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_distinct.cpp")) as f:
        host = f.read()
    for fn in ("dist_must_grow(", "dist_slots_for(", "dist_worst_vertices(", "dist_worst_edges(", "dist_vid_cap("):
        assert fn in host, fn
