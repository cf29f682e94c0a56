"""CPU: gsi::ColumnCopy, gsi::OutStage and gsi::FoldStage (csrc/gs_hostio.hpp), the one host-array
path of the stand-alone summaries, and gsi::sort_skip_above (csrc/gs_sort.hpp), in a stand-alone
program built with the address and undefined-behaviour sanitizers (tests/cpp/hostio_sanitize.cpp):
the program supplies the allocator, the copy and the stream wait itself (malloc / free / memcpy
with a call log and a failing k-th allocation) and needs no device. Beside it, the source
conditions: one driver of the one-column sort, no private staging of an export, no host-to-device
copy written out in the handles whose folds go through the fold stage."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gelly-streaming_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def _sources(pattern):
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, pattern))):
        with open(path) as f:
            out[os.path.basename(path)] = f.read()
    return out


def test_hostio_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "hostio_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + CSRC,
                            os.path.join(ROOT, "tests", "cpp", "hostio_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    # a preloaded library may precede the ASan runtime: do not treat that as an error
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_the_library_uses_the_checked_header():
    hdrs = _sources("*.hpp")
    assert '#include "gs_hostio.hpp"' in hdrs["gs_internal.hpp"]
    # only the HIP API header, standard headers, the DevBuf and the growth header: a host compiler builds the check
    includes = [ln.split()[1] for ln in hdrs["gs_hostio.hpp"].splitlines() if ln.startswith("#include")]
    assert includes == ["<hip/hip_runtime_api.h>", "<stdint.h>", '"gs_devbuf.hpp"', '"gs_grow.hpp"'], includes
    assert "GS_HIP" not in hdrs["gs_hostio.hpp"] and "fail(" not in hdrs["gs_hostio.hpp"]
    cpps = _sources("*.cpp")
    for name in ("gs_degstream.cpp", "gs_tristream.cpp", "gs_matching.cpp", "gs_distinct.cpp", "gs_slice.cpp",
                 "gs_trisample.cpp"):
        assert "ColumnCopy" in cpps[name], name
    for name in ("gs_degstream.cpp", "gs_tristream.cpp", "gs_matching.cpp", "gs_distinct.cpp", "gs_slice.cpp",
                 "gs_spanner.cpp"):
        assert "OutStage" in cpps[name], name
    for name in ("gs_degstream.cpp", "gs_tristream.cpp", "gs_matching.cpp", "gs_trisample.cpp", "gs_distinct.cpp"):
        assert "FoldStage" in cpps[name], name
    with open(os.path.join(ROOT, "gelly-streaming_amd", "Makefile")) as f:
        assert "csrc/gs_hostio.hpp" in f.read()


def test_one_driver_of_the_one_column_sort():
    cpps = _sources("*.cpp")
    users = [name for name, text in cpps.items() if "launch_sort_digits_one" in text]
    assert users == ["gs_sort.cpp"], users
    callers = {name for name, text in cpps.items() if "sort_by_key(" in text}
    assert callers == {"gs_sort.cpp", "gs_degstream.cpp", "gs_tristream.cpp", "gs_distinct.cpp", "gs_matching.cpp",
                       "gs_slice.cpp", "gs_trisample.cpp"}, callers
    # the callers' words for the error stay what they were
    for name, words in (("gs_degstream.cpp", "degstream fold"), ("gs_tristream.cpp", "tristream fold"),
                        ("gs_distinct.cpp", "distinct edges"), ("gs_matching.cpp", "matching export"),
                        ("gs_slice.cpp", "slice window"), ("gs_trisample.cpp", "trisample fold")):
        assert re.search(r'sort_by_key\([^;]*"%s"\)' % words, cpps[name]), name
    assert '": the sort ran no pass"' in cpps["gs_sort.cpp"]


def test_no_private_sort_or_staging_in_the_handles():
    for name, text in dict(_sources("*.cpp"), **_sources("*.hpp"), **_sources("*.hip")).items():
        assert not re.search(r"\b(sort_keys|ensure_staging)\s*\(", text), name
    cpps = _sources("*.cpp")
    for name in ("gs_matching.cpp", "gs_degstream.cpp", "gs_tristream.cpp", "gs_trisample.cpp"):
        assert "hipMemcpyHostToDevice" not in cpps[name], name
    # the vertex table's fold guard is written once
    guards = [name for name, text in dict(cpps, **_sources("*.hpp")).items()
              if "the fold may pass 2^31 vertex table slots" in text]
    assert guards == ["gs_vtable.hpp"], guards
