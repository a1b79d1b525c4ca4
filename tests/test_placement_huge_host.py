"""NMG_PLACE_HUGE on the CPU: the flag's accepted values, the host path
(nmg_report_placement_host, nmg_debug_object_blocks_host) over the oracle's
results of the crafted replay of test_gpu_placement.py and of a replay with a
truly huge heap object, and a stand-alone C++ program that drives the host
group walk over a [stack]-sized group.

The expectations come from the oracle's files through placement_expect.py and
placement_huge_expect.py (the rule of include/numamma_gpu.h over the cells)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import placement_expect as px
import placement_huge_expect as hx
from numamma_amd import _lib
from numamma_amd.results import _host_results, object_blocks_host, report_placement_host
from test_gpu_placement import PRIMARY, crafted_replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUGE = _lib.NMG_PLACE_HUGE
# as test_layout_host.py builds nmg_placement_host
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _read(d):
    return open(os.path.join(d, "blocks.dat")).read()


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("plh_craft"))
    rp, role = crafted_replay(d)
    raw, odir = px.run_oracle(rp, os.path.join(d, "crafted"))
    return rp, role, raw, odir


@pytest.fixture(scope="module")
def huge(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("plh_huge"))
    rp, role = hx.huge_replay()
    raw, odir = px.run_oracle(rp, os.path.join(d, "huge"))
    want = hx.check_huge_expectation(raw, rp.table, role)  # before any product code runs
    return rp, role, raw, odir, want


# ---- 1. flag values

def test_flag_values(tmp_path, crafted):
    rp, role, raw, odir = crafted
    assert HUGE == 4 and _lib.NMG_PLACE_PAGE_COUNTS | HUGE == 4
    src = tmp_path / "flag.c"
    src.write_text('#include "numamma_gpu.h"\n'
                   '_Static_assert(NMG_PLACE_HUGE == 4 && (NMG_PLACE_PAGE_COUNTS | NMG_PLACE_HUGE) == 4 && '
                   '(NMG_PLACE_PAGE_COST | NMG_PLACE_HUGE) == 6, "flag");\n'
                   "int main(void) { return 0; }\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the library; it is needed here too"
    subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)

    report_placement_host(raw, rp.table, str(tmp_path / "ok"), **PRIMARY.kw(), source=4)
    assert object_blocks_host(raw, rp.table, **PRIMARY.kw(), source=4).shape[0] > 0
    hr, keep = _host_results(raw, rp.table, np.zeros(raw.nb_buffers, dtype=np.uint64), True)
    for source in (6, 1, 3, 5, 7, 8, 1 << 32):
        with pytest.raises(_lib.NmgError) as ei:
            report_placement_host(raw, rp.table, str(tmp_path / "never"), **PRIMARY.kw(), source=source)
        assert ei.value.code == -1, source  # NMG_ERR_INVALID
        po, kmap = _lib.placement_options(raw.nb_threads, 4, PRIMARY.kw()["thread_node"], 8, source=source)
        assert _lib.lib.nmg_debug_object_blocks_host(C.byref(hr), C.byref(po), None, 0) == -1, source
    assert not os.path.exists(str(tmp_path / "never"))


# ---- 2. the crafted replay of test_gpu_placement.py

def test_crafted_replay(tmp_path, crafted):
    rp, role, raw, odir = crafted
    for o in (PRIMARY, px.Opts(2, None, 8), px.Opts(8, tuple(range(8)), 0)):
        want = hx.object_rows_all(raw, rp.table, o)
        plain = px.object_rows(raw, rp.table, o)
        got = object_blocks_host(raw, rp.table, **o.kw(), source=HUGE)
        assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), o
        st = role["stack"]
        assert np.array_equal(got[got[:, 0] != st], plain) and plain.shape[0] > 200
        assert np.array_equal(object_blocks_host(raw, rp.table, **o.kw()), plain)  # flagless: as before
        d = str(tmp_path / f"n{o.nb_nodes}")
        report_placement_host(raw, rp.table, d, **o.kw(), source=HUGE)
        assert _read(d) == px.expected_file(odir, rp.table, o), o
    got = object_blocks_host(raw, rp.table, **PRIMARY.kw(), source=HUGE)
    assert hx.blocks(got, role["stack"]) == [(0, 5, 5, 20)]


# ---- 3. a truly huge heap object

def test_huge_heap_object(tmp_path, huge):
    rp, role, raw, odir, want = huge
    o = hx.PRIMARY
    H, M = role["H"], role["M"]
    got = object_blocks_host(raw, rp.table, **o.kw(), source=HUGE)
    assert got.shape == want.shape and np.array_equal(got, want)
    plain = object_blocks_host(raw, rp.table, **o.kw())
    assert H not in plain[:, 0] and M not in plain[:, 0] and role["stack"] not in plain[:, 0]
    assert np.array_equal(plain, px.object_rows(raw, rp.table, o))
    assert np.array_equal(got[~np.isin(got[:, 0], [H, M])], plain)
    # the object is its own call site: the site's block lines are the object's blocks
    ent = rp.table.entries
    sid = {(c, s): i for i, c, s in px.read_sites(odir)}
    d = str(tmp_path / "flag")
    report_placement_host(raw, rp.table, d, **o.kw(), source=HUGE)
    text = _read(d)
    for e in (H, M):
        s = sid[(rp.table.caller(e), int(ent["initial_buffer_size"][e]))]
        assert hx.file_blocks(text, s) == hx.blocks(want, e)
    d0 = str(tmp_path / "plain")
    report_placement_host(raw, rp.table, d0, **o.kw())
    for e in (H, M):
        assert hx.file_blocks(_read(d0), sid[(rp.table.caller(e), int(ent["initial_buffer_size"][e]))]) is None
    # every other site: the file without the flag (no other entry is sparse but [stack], which no site lists)
    cut = lambda t: [b for b in t.split("#site ")[1:]
                     if int(b.split()[0]) not in {sid[(rp.table.caller(e), int(ent["initial_buffer_size"][e]))] for e in (H, M)}]
    assert cut(text) == cut(_read(d0)) and len(cut(text)) > 20


# ---- 4. the host group walk, stand-alone under the sanitizers

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
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert name + ": ok" in r.stdout
    return r.stdout, ""


def test_group_walk_standalone(tmp_path):
    out, err = _build_and_run("nmg_placement_huge_host", str(tmp_path), SAN)
    if out is None:  # a compiler without the sanitizer runtimes: the same checks, plain
        out, err = _build_and_run("nmg_placement_huge_host", str(tmp_path))
    assert out is not None, err
