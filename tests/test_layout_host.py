"""The counter arrays' layout and the page-cell placement on the CPU.

numamma_amd/csrc/nmg_internal.h is the one description of the flat counter
arrays (sum64 / min64 / max64) and holds the rule that places an entry's page
cells; it needs no HIP.  Two stand-alone programs under tests/c include it,
compiled with g++ and run as child processes:

  nmg_layout_host     prints every constant and word count, compared here
                      with the Python mirror (numamma_amd/results.py), and
                      checks that the index helpers tile each array;
  nmg_placement_host  drives CellCursor through the dense case and each of
                      its limits, under the address and undefined-behaviour
                      sanitizers where the compiler has them (linked
                      statically: the test preloads nothing).
"""
import os
import shutil
import subprocess

from numamma_amd import results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _build_and_run(name, d, extra=(), args=()):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = os.path.join(d, name)
    r = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", *extra,
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "numamma_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    if r.returncode:
        return None, r.stderr
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert name + ": ok" in r.stdout
    return r.stdout, ""


def test_layout_matches_python_mirror(tmp_path):
    out, err = _build_and_run("nmg_layout_host", str(tmp_path))
    assert out is not None, err
    got = dict(line.split() for line in out.splitlines() if not line.endswith(": ok"))
    want = {name: getattr(results, name) for name in ("NB_BUCKETS", "GLOBAL_SUMS", "LEVEL_WORDS", "GLOBAL_SUM_WORDS",
                                                      "CW_ROWS", "GLOBAL_MIN_WORDS", "COUNTER_WORDS")}
    want["max64_words"] = results.max64_words()
    for E in (0, 1, 5):
        want[f"min64_words:{E}"] = results.min64_words(E)
        for levels in (0, 1):
            want[f"sum64_words:{E}:{levels}"] = results.sum64_words(E, bool(levels))
    assert {k: int(v) for k, v in got.items()} == want
    # the raw dump's records follow from the same names
    assert results.ENTRY_WORDS == 1 + results.GLOBAL_SUM_WORDS
    assert results.COUNTER_WORDS == results.GLOBAL_SUMS + results.GLOBAL_MIN_WORDS


def test_cell_placement(tmp_path):
    out, err = _build_and_run("nmg_placement_host", str(tmp_path), SAN)
    if out is None:  # a compiler without the sanitizer runtimes: the same checks, plain
        out, err = _build_and_run("nmg_placement_host", str(tmp_path))
    assert out is not None, err
