"""CPU: gsi::Event, Stream, HostBuf and SpanTimer (csrc/gs_own.hpp), the owner types of every HIP
event, stream and pinned host block of the handles, in a stand-alone program built with the
address and undefined-behaviour sanitizers (tests/cpp/own_sanitize.cpp): the program supplies the
HIP calls itself (malloc / free with live sets, a release log and a failing k-th creating call)
and needs no device. And the structure that makes the check cover the library: nothing else
under csrc/ creates or releases such a resource."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gelly-streaming_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_owners_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "own_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + CSRC,
                            os.path.join(ROOT, "tests", "cpp", "own_sanitize.cpp"), "-o", exe],
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
    with open(os.path.join(CSRC, "gs_internal.hpp")) as f:
        assert '#include "gs_own.hpp"' in f.read()
    with open(os.path.join(CSRC, "gs_own.hpp")) as f:
        text = f.read()
    # only the HIP API header and standard headers: a host compiler builds the check above
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<hip/hip_runtime_api.h>", "<stddef.h>", "<string.h>", "<utility>", "<vector>"], includes
    with open(os.path.join(ROOT, "gelly-streaming_amd", "Makefile")) as f:
        hdrs = [ln for ln in f.read().splitlines() if ln.startswith("HDRS")]
    assert len(hdrs) == 1 and "csrc/gs_own.hpp" in hdrs[0].split()


def test_only_the_owner_types_create_and_release():
    """Calls (a name followed by `(`) of the create / destroy / free functions occur in gs_own.hpp
    and in gs_ingest.hip (the thread-local ParseCache, see the header's comment) alone."""
    calls = re.compile(r"\b(hipEventCreate|hipEventDestroy|hipStreamCreate|hipStreamDestroy|hipHostMalloc|"
                       r"hipHostFree|hipHostGetDevicePointer)\w*\s*\(")
    found = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            hits = sorted({m.group(1) for m in calls.finditer(f.read())})
        if hits:
            found[name] = hits
    assert set(found) == {"gs_own.hpp", "gs_ingest.hip"}, found
