"""CPU: gsi::grow_group / gsi::alloc_each (csrc/gs_grow.hpp), the one way a handle grows a group
of device buffers, in a stand-alone program built with the address and undefined-behaviour
sanitizers (tests/cpp/grow_sanitize.cpp): the program supplies the allocator and the stream wait
itself (malloc / free with a live-byte count, a call log, a failing k-th allocation, a failing
wait) and needs no device. Beside it, the source conditions of the handle skeleton: one null
check, one truncation error, one launch-check macro, one Python owner of the handle lifecycle."""
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


def test_grow_group_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "grow_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + CSRC,
                            os.path.join(ROOT, "tests", "cpp", "grow_sanitize.cpp"), "-o", exe],
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
    assert '#include "gs_grow.hpp"' in hdrs["gs_internal.hpp"]
    # only the HIP API header, standard headers and the DevBuf header: a host compiler builds the check above
    includes = [ln.split()[1] for ln in hdrs["gs_grow.hpp"].splitlines() if ln.startswith("#include")]
    assert includes == ["<hip/hip_runtime_api.h>", "<stdint.h>", '"gs_devbuf.hpp"'], includes
    assert "GS_HIP" not in hdrs["gs_grow.hpp"] and "fail(" not in hdrs["gs_grow.hpp"]
    users = [name for name, text in _sources("*.cpp").items() if "grow_group(" in text]
    assert set(users) >= {"gs_slice.cpp", "gs_triangle.cpp", "gs_distinct.cpp", "gs_spanner.cpp", "gs_matching.cpp",
                          "gs_capi.cpp"}, users
    with open(os.path.join(ROOT, "gelly-streaming_amd", "Makefile")) as f:
        assert "csrc/gs_grow.hpp" in f.read()


def test_one_null_check_one_truncation_error_one_launch_check():
    text = dict(_sources("*.cpp"), **_sources("*.hpp"))
    for name, t in text.items():
        assert not re.search(r"\bint check_(mt|sp|tri|slice|distinct)\(", t), name
    defs = [name for name, t in text.items() if re.search(r"^(inline )?int truncated\(", t, re.M)]
    assert defs == ["gs_internal.hpp"], defs
    # a launch is checked through GS_LAUNCH; what remains bare does not follow a launch directly: the six sites
    # of gs_capi.cpp where a profiling span closes between the launch and its check
    bare = {name: len(re.findall(r"^\s*GS_HIP\(hipGetLastError\(\)\);", t, re.M))
            for name, t in _sources("*.cpp").items()}
    assert {k: v for k, v in bare.items() if v} == {"gs_capi.cpp": 6}, bare
    for m in re.finditer(r"^(.*)\n\s*GS_HIP\(hipGetLastError\(\)\);", text["gs_capi.cpp"], re.M):
        assert m.group(1).strip() == "}", m.group(1)


def test_one_python_class_owns_the_handle_lifecycle():
    import gsamd
    for name in ("Summary", "Degrees", "Triangles", "Slice", "Distinct", "Spanner", "Matching"):
        cls = getattr(gsamd, name)
        assert "__del__" not in vars(cls) and "close" not in vars(cls), name
        assert cls.__del__ is gsamd._Handle.__del__, name
