"""NMG_COST_SCOPE_ALL on the CPU: the entry point and its constants, the
expectation helper's self-check against the oracle alone (cost_all_expect.py),
and nmg_report_page_cost_host over rows that include sparse entries."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cost_all_expect as ax
import cost_expect as cx
import placement_huge_expect as hx
from numamma_amd import _lib
from numamma_amd.replay import SynthConfig, generate
from numamma_amd.results import report_page_cost_host
from test_gpu_placement_huge import T, _mid_budget, dense_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_and_exported():
    assert "nmg_set_page_cost_ex" in _lib.declared_symbols()
    assert hasattr(_lib.lib, "nmg_set_page_cost_ex")
    assert _lib.lib.nmg_set_page_cost_ex(None, None, 0) == -1
    o = _lib.nmg_page_cost_options(cx.MEMORY, 3, cx.WEIGHT, 0, 0)
    assert _lib.lib.nmg_set_page_cost_ex(None, C.byref(o), _lib.NMG_COST_SCOPE_ALL) == -1


def test_constants(tmp_path):
    assert (_lib.NMG_COST_SCOPE_DENSE, _lib.NMG_COST_SCOPE_ALL) == (0, 1) == (ax.SCOPE_DENSE, ax.SCOPE_ALL)
    assert C.sizeof(_lib.nmg_page_cost_options) == 24  # (the options keep their layout)
    src = tmp_path / "scope.c"
    src.write_text('#include "numamma_gpu.h"\n'
                   "_Static_assert(NMG_COST_SCOPE_DENSE == 0 && NMG_COST_SCOPE_ALL == 1, \"scope\");\n"
                   "_Static_assert(sizeof(struct nmg_page_cost_options) == 24, \"size\");\n"
                   "int (*entry)(nmg_engine *, const struct nmg_page_cost_options *, uint32_t) = nmg_set_page_cost_ex;\n"
                   "int main(void) { return entry == 0; }\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the library; it is needed here too"
    subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_selected_levels_property():
    """SELECTED: exactly the levels with a HIT or MISS and a level bit, or NA (asserted inside from sel())."""
    L = ax.selected_levels()
    assert L == ax.SELECTED and cx.LVL_NA in L and 0 not in L and cx.LVL_L2 not in L
    assert ax.sel(cx.LVL_HIT | cx.LVL_MISS | cx.LVL_L3) == 1 << 2  # HIT beats MISS
    assert ax.sel(cx.LVL_MISS | cx.LVL_REM_RAM1 | cx.LVL_REM_RAM2) == 1 << (9 + 5)  # one bucket, once
    assert ax.sel(cx.LVL_NA | cx.LVL_MISS | cx.LVL_LOC_RAM) == cx.NA | 1 << (9 + 4)


def test_helper_covers_every_cell_of_the_huge_replay(tmp_path):
    """The all-true Dump's lines plus [stack]'s page cells are the oracle's page
    cells: with H, M (sparse by the per-entry cap) and the stack's planted page."""
    rp, role = hx.huge_replay(stack=True)
    raw, odir = cx.run_oracle(rp, str(tmp_path / "o"))
    dump = ax.DumpAll(odir, rp.table, rp.nb_threads)
    st = role["stack"]
    assert ax.stack_entry(rp.table) == st
    assert ax.check_dump_covers(dump, raw, rp.table) >= 1
    cells = raw.cells
    assert int(cells[cells[:, 0] == st][:, 3].sum()) >= 20
    ok = cx.dense(rp.table, rp.nb_threads)
    assert not ok[role["H"]] and not ok[role["M"]] and not ok[st]
    # the scoped rows hold H and M; the dense-scope rows (cost_expect's own) do not
    rows = dump.rows(cx.EVERYTHING)[0]
    dense_rows = dump.dense_rows(cx.EVERYTHING)
    assert np.array_equal(dense_rows, cx.Dump(odir, rp.table, rp.nb_threads).rows(cx.EVERYTHING)[0])
    assert np.array_equal(rows[ok[rows[:, 0].astype(np.int64)]], dense_rows)
    for e in (role["H"], role["M"]):
        assert (rows[:, 0] == e).any() and not (dense_rows[:, 0] == e).any()
    assert not (rows[:, 0] == st).any()


@pytest.mark.parametrize("o", [cx.MEMORY_WEIGHT, cx.EVERYTHING], ids=["memory-weight", "all-count"])
def test_report_host_with_sparse_members(tmp_path, o):
    """Rows of every entry -- at the mid budget some members of non-stack sites
    are sparse -- give each site the file of the oracle's per-site dump, which
    holds every non-stack member; the dense rows alone leave such a site short."""
    rp = generate(SynthConfig(nb_samples=60_000, nb_intervals=1_500, seed=102))
    assert rp.nb_threads == T
    raw, odir = cx.run_oracle(rp, str(tmp_path / "o"))
    table = rp.table
    dump = ax.DumpAll(odir, table, rp.nb_threads)
    rows = dump.rows(o)[0]
    dm = dense_model(table, T, _mid_budget(table))
    sparse_rows = rows[~dm[rows[:, 0].astype(np.int64)]]
    assert sparse_rows.shape[0] > 100 and dm[rows[:, 0].astype(np.int64)].sum() > 100
    want = cx.site_files(cx.site_matrices(odir, rp.nb_threads, o))
    d = str(tmp_path / "all")
    report_page_cost_host(raw, table, d, rows)
    assert cx.read_dir(d, "") == want and len(want) > 50
    # the sparse members' rows matter: without them some site's file differs or is missing
    d2 = str(tmp_path / "dense")
    report_page_cost_host(raw, table, d2, rows[dm[rows[:, 0].astype(np.int64)]])
    short = cx.read_dir(d2, "")
    changed = [n for n in want if short.get(n) != want[n]]
    assert changed and all(os.path.exists(os.path.join(d, n)) for n in changed)
