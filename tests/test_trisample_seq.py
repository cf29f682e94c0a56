"""CPU: the sampling triangle estimate's rules header (csrc/gs_trisample_seq.hpp: java.util.Random's
LCG and its jump-ahead, the coin, the third-vertex draw, the candidate record, the estimate with
Java's int cast, the lane functions of the kernels, the sequential definition and the fold by
parts) in a stand-alone program built with the address and undefined-behaviour sanitizers
(tests/cpp/trisample_seq_sanitize.cpp): three published values of java.util.Random and the pins of
tests/golden/trisample_pins.json, the jump against stepping, the cast, ts_fold_parts against
ts_fold_seq under chunk and tile sizes 1, 2, 64 and n. The header is the one the kernels include."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gelly-streaming_amd", "csrc")


def test_rules_and_decomposition_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "trisample_seq_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + CSRC,
                            os.path.join(ROOT, "tests", "cpp", "trisample_seq_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    # a preloaded library may precede the ASan runtime: do not treat that as an error
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    # the values the program printed are the committed pins
    got = {}
    for line in run.stdout.splitlines():
        if line.startswith("PIN "):
            name, *vals = line.split()[1:]
            got[name] = vals
    with open(os.path.join(ROOT, "tests", "golden", "trisample_pins.json")) as f:
        pins = json.load(f)
    assert int(got["random0_next_int"][0]) == pins["java"]["random0_next_int"] == -1155484576
    assert int(got["random42_next_int"][0]) == pins["java"]["random42_next_int"] == -1170105035
    assert float(got["random0_next_double"][0]) == pins["java"]["random0_next_double"] == 0.730967787376657
    assert pins["master_seed"] == -559038737
    assert [int(x) for x in got["instance_seeds"]] == pins["instance_seeds"]
    assert pins["instance_seeds"][:2] == [993338671, -758524624] and len(pins["instance_seeds"]) == 8
    assert pins["coin_limit"] == 2000 and len(pins["coin_successes"]) == 4
    for i, want in enumerate(pins["coin_successes"]):
        assert [int(x) for x in got["coin_successes_%d" % i]] == want
    assert pins["coin_successes"][0] == [1, 3, 7, 40, 470]
    k5 = pins["k5_twice"]
    rows = [int(x) for x in got["k5_rows"]]
    assert [rows[i:i + 2] for i in range(0, len(rows), 2)] == k5["rows"] == [[8, 6], [13, 19], [15, 11], [16, 24],
                                                                               [19, 42]]
    assert int(got["k5_beta_sum"][0]) == k5["beta_sum"] == 3
    assert int(got["k5_max_attempts"][0]) == k5["max_attempts"] == 4
    for i, want in enumerate(k5["states"]):
        assert [int(x) for x in got["k5_state_%d" % i]] == [int(x) for x in want]
    assert k5["states"][2] == [0, 3, 1, False, True, 0, 13]


def test_kernels_and_host_include_the_checked_header():
    with open(os.path.join(CSRC, "gs_trisample.hpp")) as f:
        hpp = f.read()
    assert '#include "gs_trisample_seq.hpp"' in hpp
    assert not any("scan" in ln for ln in hpp.splitlines() if ln.startswith("void launch_"))
    with open(os.path.join(CSRC, "gs_trisample_k.hip")) as f:
        text = f.read()
    assert '#include "gs_trisample.hpp"' in text and '#include "gs_scan.hpp"' in text
    for fn in ("ts_jump(", "ts_apply(", "ts_coin_lane(", "ts_instance_state(", "ts_state_init(", "ts_seg_carried(",
               "ts_seg_sampled(", "ts_search_lane(", "ts_outcome(", "ts_state_of(", "ts_estimate(",
               "block_excl_scan<", "block_count_to<"):
        assert fn in text, fn
    assert "wave_incl_scan(uint32_t" not in text
    with open(os.path.join(CSRC, "gs_trisample.cpp")) as f:
        host = f.read()
    assert '#include "gs_trisample.hpp"' in host
    for fn in ("kTsChunk", "kTsTile", "kTsMaxFold", "kTsMaxSamples", "kTsMaxVertices", "kTsMaxArrivals",
               "launch_tile_scan(", "sort_by_key(", "grow_group(", "check_handle(", "truncated(", "owner_create("):
        assert fn in host, fn
    with open(os.path.join(CSRC, "gs_trisample_seq.hpp")) as f:
        seq = f.read()
    # the fold by parts is made of the lane functions the kernels call
    for fn in ("ts_coin_lane(", "ts_seg_carried(", "ts_seg_sampled(", "ts_search_lane(", "ts_outcome(", "ts_state_of(",
               "ts_estimate(", "ts_third(", "ts_coin_rejects("):
        assert seq.count(fn) >= 2, fn
    assert "inline void ts_fold_seq(" in seq and "inline void ts_fold_parts(" in seq
    assert "Not built: parallelism above 1" in seq and "intermediate emissions" in seq
    # the header itself reads standard headers only (and the HIP runtime under a HIP compiler)
    incs = [ln.split()[1] for ln in seq.splitlines() if ln.startswith("#include")]
    assert all(i.startswith("<") for i in incs), incs
    with open(os.path.join(ROOT, "gelly-streaming_amd", "Makefile")) as f:
        mk = f.read()
    for word in ("csrc/gs_trisample.hpp", "csrc/gs_trisample_seq.hpp", "gs_trisample_k.o", "gs_trisample.o"):
        assert word in mk, word
