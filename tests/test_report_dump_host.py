"""The report writer's files on the CPU: tests/c/nmg_report_dump_host.cpp drives
nmg::write_report (every dump mode, over a DumpInput that only the engine
builds otherwise), write_timeline, write_page_cost and write_blocks, compares
every file with the bytes written out in the program, and takes every error
return with its text, the files it leaves and the descriptors it leaves open.

Built with nmg_report.cpp as test_placement_huge_host.py builds its program:
under the address and undefined-behaviour sanitizers (leak detection on) where
the compiler has them.  The GPU suites compare the same files with the oracle
end to end; this is the fast pin."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _build_and_run(name, d, extra=()):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = os.path.join(d, name)
    r = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", *extra,
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "numamma_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", name + ".cpp"),
                        os.path.join(ROOT, "numamma_amd", "csrc", "nmg_report.cpp"), "-o", exe, "-pthread"],
                       capture_output=True, text=True)
    if r.returncode:
        return None, r.stderr
    run = os.path.join(d, "run" + ("_san" if extra else ""))  # the program writes under its working directory
    os.mkdir(run)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, cwd=run)
    assert r.returncode == 0, r.stdout + r.stderr
    assert name + ": ok" in r.stdout
    return r.stdout, ""


def test_report_files_standalone(tmp_path):
    out, err = _build_and_run("nmg_report_dump_host", str(tmp_path), SAN)
    if out is None:  # a compiler without the sanitizer runtimes: the same checks, plain
        out, err = _build_and_run("nmg_report_dump_host", str(tmp_path))
    assert out is not None, err
