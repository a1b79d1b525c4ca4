"""nmg_report_page_cost_host on the CPU: the oracle's raw results plus cost rows
built in numpy from its all_memory_accesses.dat give, per call site, a
callsite_cost_<id>.dat equal to the oracle's callsite_dump_<id>.dat selected
and summed by the same rule (cost_expect.py) -- the matrix of
callsite_counters_<id>.dat, the same site ids.  Also the argument errors, the
struct's size and its ctypes mirror."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cost_expect as cx
from numamma_amd import _lib
from numamma_amd.replay import SynthConfig, generate
from numamma_amd.results import report_host, report_page_cost_host, report_placement_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    rp = generate(SynthConfig(nb_samples=20_000, nb_intervals=300, nb_threads=4, seed=101))
    raw, odir = cx.run_oracle(rp, str(tmp_path_factory.mktemp("costhost")))
    dump = cx.Dump(odir, rp.table, rp.nb_threads)
    rows, nsel = dump.rows(cx.CostOpts(cx.MEMORY, 3, cx.COUNT))
    assert (dump.nlines, nsel, rows.shape[0], dump.unknown) == (16_968, 1_699, 781, 182)
    return rp, raw, odir, dump


@pytest.mark.parametrize("o", cx.OPTION_SETS, ids=cx.OPTION_IDS)
def test_site_files_match_selected_oracle_dumps(tmp_path, case, o):
    rp, raw, odir, dump = case
    rows, nsel = dump.rows(o)
    want = cx.site_files(cx.site_matrices(odir, rp.nb_threads, o))
    assert nsel > 100 and len(want) > 10
    pdir = str(tmp_path / "product")
    report_page_cost_host(raw, rp.table, pdir, rows)
    assert cx.read_dir(pdir, "") == want  # (nothing but the cost files is written)
    # the ids and the matrix shape are nmg_report_host's for the same results
    rdir = str(tmp_path / "report")
    report_host(raw, rp.table, np.zeros(raw.nb_buffers, dtype=np.uint64), rdir, str(tmp_path / "p.txt"))
    for name, text in want.items():
        counters = open(os.path.join(rdir, name.replace("callsite_cost_", "callsite_counters_"))).read()
        assert [len(l.split("\t")) for l in text.splitlines()] == [len(l.split("\t")) for l in counters.splitlines()]
    # shuffled rows, and a cell given in two parts, give the same files
    big = rows[rows[:, 3] > 1]
    part = big.copy()
    part[:, 3] = 1
    rest = rows.copy()
    rest[rows[:, 3] > 1, 3] -= np.uint64(1)
    mixed = np.concatenate([rest, part])
    mixed = mixed[np.random.default_rng(5).permutation(mixed.shape[0])]
    shutil.rmtree(pdir)
    report_page_cost_host(raw, rp.table, pdir, mixed)
    assert cx.read_dir(pdir, "") == want


def test_all_buckets_are_the_counter_files_minus_unknown(tmp_path, case):
    """Every bucket and N/A, both accesses, counted: the oracle's own
    callsite_counters_<id>.dat less the level-0 lines."""
    rp, raw, odir, dump = case
    mats = cx.site_matrices(odir, rp.nb_threads, cx.EVERYTHING)
    import placement_expect as px
    short = 0
    for sid, m in mats.items():
        full = px.site_matrix(odir, sid)
        assert full.shape == m.shape and (m <= full).all()
        short += int((full - m).sum())
    assert short == dump.unknown


def test_argument_errors(tmp_path, case):
    rp, raw, odir, dump = case
    rows, _ = dump.rows(cx.MEMORY_WEIGHT)
    d = str(tmp_path / "x")
    for bad in ((0, raw.nb_entries), (1, rp.nb_threads)):  # an entry / a thread out of range
        r = rows.copy()
        r[3, bad[0]] = bad[1]
        with pytest.raises(_lib.NmgError) as ei:
            report_page_cost_host(raw, rp.table, d, r)
        assert ei.value.code == -1
    lib = _lib.lib
    assert lib.nmg_report_page_cost_host(None, None, None, None, 0) == -1
    from numamma_amd.results import _host_results
    hr, keep = _host_results(raw, rp.table, np.zeros(raw.nb_buffers, dtype=np.uint64), True)
    assert lib.nmg_report_page_cost_host(C.byref(hr), None, None, None, 0) == -1  # entries without meta
    from numamma_amd.engine import build_meta
    meta, kmeta = build_meta(rp.table)
    ro = _lib.nmg_report_options(d.encode(), 1, 0, None, None, None, 0, 0)
    assert lib.nmg_report_page_cost_host(C.byref(hr), meta, C.byref(ro), None, 5) == -1  # rows missing
    assert lib.nmg_report_page_cost_host(C.byref(hr), meta, C.byref(ro), None, -1) == -1
    assert lib.nmg_report_page_cost_host(C.byref(hr), meta, C.byref(ro), None, 0) == 0  # no rows: no files
    assert cx.read_dir(d, "") == {}
    del keep, kmeta
    ro = _lib.nmg_report_options(str(tmp_path / "ro" / "nested").encode(), 1, 0, None, None, None, 0, 0)
    hr, keep = _host_results(raw, rp.table, np.zeros(raw.nb_buffers, dtype=np.uint64), True)
    r = np.ascontiguousarray(rows)
    assert lib.nmg_report_page_cost_host(C.byref(hr), meta, C.byref(ro), r.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         r.shape[0]) == -10  # NMG_ERR_IO: the directory cannot be made
    del keep


def test_placement_host_rejects_the_cost_source(tmp_path, case):
    rp, raw, odir, dump = case
    from numamma_amd.results import _host_results
    from numamma_amd.engine import build_meta
    hr, keep = _host_results(raw, rp.table, np.zeros(raw.nb_buffers, dtype=np.uint64), True)
    meta, kmeta = build_meta(rp.table)
    ro = _lib.nmg_report_options(str(tmp_path).encode(), 1, 0, None, None, None, 0, 0)
    for source, rc in ((_lib.NMG_PLACE_PAGE_COST, -1), (1, -1), (3, -1), (_lib.NMG_PLACE_PAGE_COUNTS, 0)):
        po, kmap = _lib.placement_options(rp.nb_threads, 2, source=source)
        assert _lib.lib.nmg_report_placement_host(C.byref(hr), meta, C.byref(ro), C.byref(po)) == rc, source
    with pytest.raises(ValueError):
        _lib.placement_options(rp.nb_threads, 2, reserved=1, source=2)
    assert _lib.placement_options(rp.nb_threads, 2, reserved=1)[0].source == 1  # the field's earlier name
    del keep, kmeta
    report_placement_host(raw, rp.table, str(tmp_path / "again"), 2)  # (the count source, as before)


def test_struct_size_and_mirror(tmp_path):
    o = _lib.nmg_page_cost_options
    assert C.sizeof(o) == 24
    assert [(n, getattr(o, n).offset, getattr(o, n).size) for n, _ in o._fields_] == [
        ("bucket_mask", 0, 4), ("access_mask", 4, 4), ("metric", 8, 4), ("reserved", 12, 4), ("budget_bytes", 16, 8)]
    assert (_lib.NMG_COST_COUNT, _lib.NMG_COST_WEIGHT, _lib.NMG_COST_NA, _lib.NMG_COST_REMOTE, _lib.NMG_COST_MEMORY,
            _lib.NMG_PLACE_PAGE_COUNTS, _lib.NMG_PLACE_PAGE_COST) == (0, 1, 0x40000, 0x60, 0x70, 0, 2)
    assert (cx.NA, cx.REMOTE, cx.MEMORY) == (_lib.NMG_COST_NA, _lib.NMG_COST_REMOTE, _lib.NMG_COST_MEMORY)
    # the header itself, as a C99 compiler lays it out
    src = tmp_path / "size.c"
    src.write_text(
        '#include <stddef.h>\n#include "numamma_gpu.h"\n'
        "_Static_assert(sizeof(struct nmg_page_cost_options) == 24, \"size\");\n"
        "_Static_assert(offsetof(struct nmg_page_cost_options, budget_bytes) == 16, \"budget\");\n"
        "_Static_assert(sizeof(struct nmg_placement_options) == 24 && "
        "offsetof(struct nmg_placement_options, source) == 16, \"placement\");\n"
        "_Static_assert(NMG_COST_COUNT == 0 && NMG_COST_WEIGHT == 1 && NMG_COST_NA == 0x40000u && "
        "NMG_COST_REMOTE == 0x60u && NMG_COST_MEMORY == 0x70u && NMG_PLACE_PAGE_COUNTS == 0 && "
        "NMG_PLACE_PAGE_COST == 2, \"constants\");\n"
        "int main(void) { return 0; }\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the library; it is needed here too"
    subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
