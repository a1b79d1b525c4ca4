"""The engine's owning buffer types (numamma_amd/csrc/nmg_buffer.h) on the CPU.

tests/c/nmg_buffer_host.cpp defines the four HIP allocation functions itself,
over malloc, so DevBuf / PinBuf run without a GPU: compiled with g++ and the
address + undefined-behaviour sanitizers, run as a child process (the test
preloads nothing into it).  The program asserts the contract (reserve grows once and only past
the capacity, a failed allocation leaves the buffer empty with the old block
freed once, moves leave the source empty, alloc(0) yields a pointer, the
destructor frees, no block is live at exit); the sanitizers catch what it
cannot (a double free, a leak)."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
# (the runtimes linked statically: the program then starts whatever the
# environment preloads, and the test itself preloads nothing)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _sanitizers_missing(cxx, d):
    """A reason string when `cxx` cannot link a sanitized program, else None."""
    src = os.path.join(d, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, src, "-o", os.path.join(d, "probe")], capture_output=True, text=True)
    return None if r.returncode == 0 else "the compiler lacks the sanitizer runtime: " + r.stderr.strip()[-200:]


def test_buffer_types_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    assert glob.glob(os.path.join(ROCM_INC, "hip", "hip_runtime_api.h")), "ROCm headers not found"
    d = str(tmp_path)
    why = _sanitizers_missing(cxx, d)
    if why:
        pytest.skip(why)
    exe = os.path.join(d, "nmg_buffer_host")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", *SAN, "-D__HIP_PLATFORM_AMD__", "-I", ROCM_INC,
                        "-I", os.path.join(ROOT, "numamma_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", "nmg_buffer_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nmg_buffer_host: ok" in r.stdout
