"""NMG_TL_SCOPE_ALL on the CPU: the entry point and its constants, the
expectation helper's self-check against the oracle alone
(timeline_all_expect.py), the timeline sparse table's key and the host merge
of its rows (tests/c/nmg_tl_sparse_host.cpp, a stand-alone program under the
address and undefined-behaviour sanitizers), and nmg_report_timeline_host over
rows that include sparse entries and [stack]."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import timeline_all_expect as ax
import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd.results import report_timeline_host
from test_layout_host import SAN, _build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = tx.TlOpts()


def test_entry_point_declared_and_exported():
    assert "nmg_set_timeline_ex" in _lib.declared_symbols()
    assert hasattr(_lib.lib, "nmg_set_timeline_ex")
    assert _lib.lib.nmg_set_timeline_ex(None, None, 0) == -1
    o = _lib.nmg_timeline_options(OPTS.t0, OPTS.bin_shift, OPTS.nb_bins, 0, 0, 4096, 0)
    assert _lib.lib.nmg_set_timeline_ex(None, C.byref(o), _lib.NMG_TL_SCOPE_ALL) == -1


def test_constants(tmp_path):
    assert (_lib.NMG_TL_SCOPE_DENSE, _lib.NMG_TL_SCOPE_ALL) == (0, 1) == (ax.SCOPE_DENSE, ax.SCOPE_ALL)
    # the options keep their layout: 8 + 4 * 4 + 8 + 8 = 40 bytes, as before the scope existed
    assert C.sizeof(_lib.nmg_timeline_options) == 40
    src = tmp_path / "scope.c"
    src.write_text('#include "numamma_gpu.h"\n'
                   "_Static_assert(NMG_TL_SCOPE_DENSE == 0 && NMG_TL_SCOPE_ALL == 1, \"scope\");\n"
                   "_Static_assert(sizeof(struct nmg_timeline_options) == 40, \"size\");\n"
                   "int (*entry)(nmg_engine *, const struct nmg_timeline_options *, uint32_t) = nmg_set_timeline_ex;\n"
                   "int main(void) { return entry == 0; }\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the library; it is needed here too"
    subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_key_and_merge_program(tmp_path):
    """tests/c/nmg_tl_sparse_host.cpp: the key round trip at every field's
    limits, never the all-ones word, and the merge of sparse rows into dense rows."""
    out, err = _build_and_run("nmg_tl_sparse_host", str(tmp_path), SAN)
    if out is None:  # a compiler without the sanitizer runtimes: the same checks, plain
        out, err = _build_and_run("nmg_tl_sparse_host", str(tmp_path))
    assert out is not None, err


def test_key_mirror():
    """The numpy mirror: the layout's words, round trip at the limits, key order = row order."""
    assert int(ax.tl_key(1022, 4095, 1023, 0xFFFFFFFF)) == 0xFFBFFFFFFFFFFFFF
    assert int(ax.tl_key(1, 0, 0, 0)) == 1 << 54 and int(ax.tl_key(0, 1, 0, 0)) == 1 << 42
    assert int(ax.tl_key(0, 0, 1, 0)) == 1 << 32 and int(ax.tl_key(0, 0, 0, 1)) == 1
    f = [np.array(v, dtype=np.uint64) for v in ([0, 1022, 7, 1022], [0, 4095, 9, 0], [0, 1023, 3, 1023], [0, 0xFFFFFFFF, 5, 1])]
    k = ax.tl_key(*f)
    assert all(np.array_equal(a, b) for a, b in zip(ax.tl_key_fields(k), f))
    assert not (k == np.uint64(0xFFFFFFFFFFFFFFFF)).any()
    rng = np.random.default_rng(5)
    rows = np.stack([rng.integers(0, 1023, 500), rng.integers(0, 4096, 500), rng.integers(0, 1024, 500),
                     rng.integers(0, 1 << 32, 500)], axis=1).astype(np.uint64)
    by_rows = np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))
    assert np.array_equal(np.argsort(ax.tl_key(*rows.T), kind="stable"), by_rows)


@pytest.fixture(scope="module")
def huge(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tla_huge"))
    rp, role = ax.huge_replay_tl(OPTS)
    raw, odir = tx.run_oracle(rp, d)
    return rp, role, raw, odir


def test_helper_covers_every_cell_of_the_huge_replay(huge):
    """On the oracle's files alone: H's rows span at least four bins, bin 0
    through a ts < t0 sample and the last bin through the clamp, every
    timestamp inside H's life; the rows summed over the bins are the oracle's
    page cells of every selected entry, H, M and [stack] included."""
    rp, role, raw, odir = huge
    table = rp.table
    ent = table.entries
    H, M, st = role["H"], role["M"], role["stack"]
    assert ax.stack_entry(table) == st
    o = OPTS
    a = tx._columns(os.path.join(odir, "all_memory_accesses.dat"), 4)  # thread ts object_id offset
    h = a[ax._entry_of_lines(a, table) == H]
    al, fr = int(ent["alloc_date"][H]), int(ent["free_date"][H])
    assert h.shape[0] > 200 and int(h[:, 1].min()) >= al and int(h[:, 1].max()) <= fr
    assert int(h[:, 1].min()) < o.t0  # a sample from before t0: bin 0
    assert int(h[:, 1].max()) >= o.t0 + (o.nb_bins << o.bin_shift)  # one past the last bin's end: the clamp
    assert set(np.unique(tx.bins_of(h[:, 1], o)).tolist()) == {0, 3, 6, o.nb_bins - 1}
    rows = ax.expected_rows_all(odir, raw, table, o)
    hb = set(rows[rows[:, 0] == H][:, 1].tolist())
    assert len(hb) >= 4 and {0, o.nb_bins - 1} <= hb
    assert len(set(rows[rows[:, 0] == M][:, 1].tolist())) >= 2
    srows = rows[rows[:, 0] == st]
    assert srows.shape[0] >= 1 and (srows[:, 1] == 0).all() and int(srows[:, 4].sum()) >= 20
    assert (srows[:, 3] == ax.hx.STACK_PAGE).any()  # a row past 2^26
    cells = ax.check_covers(rows, raw, table, o)
    assert all((cells[:, 0] == e).any() for e in (H, M, st))
    # the dense scope's rows are the rows of the entries the per-entry cap leaves dense
    dense = tx.selected(table, rp.nb_threads, o)
    want_dense, _ = tx.expected_rows(odir, table, rp.nb_threads, o)
    assert np.array_equal(rows[dense[rows[:, 0]]], want_dense)
    assert not dense[H] and not dense[M] and not dense[st]
    ids = want_dense[:, 0]
    assert (ids < M).any() and ((ids > M) & (ids < H)).any()  # dense entries on both sides of M
    # coarser rows: the same cover
    c = tx.TlOpts(row_shift=3)
    ax.check_covers(ax.expected_rows_all(odir, raw, table, c), raw, table, c)
    # the keys of the sparse rows: three ordinals, ascending with the rows
    k = ax.sparse_keys(rows, table, dense, o)
    assert set(ax.tl_key_fields(k)[0].tolist()) == {0, 1, 2} and k.shape[0] == int((~dense[rows[:, 0]]).sum())


def test_report_host_with_sparse_members(tmp_path, huge):
    """Rows that include H, M and [stack] give each site the file of the
    oracle's per-site dump: H's and M's own sites too, none for the stack."""
    rp, role, raw, odir = huge
    table = rp.table
    o = OPTS
    want = tx.expected_site_files(odir, o)
    # (the oracle's per-site dumps hold every member: rows of every entry, min_object_bytes = 0)
    every = tx.TlOpts(min_object_bytes=0)
    rows0 = ax.expected_rows_all(odir, raw, table, every)
    d0 = str(tmp_path / "every")
    report_timeline_host(raw, table, d0, rows0, **every.kw())
    got = tx.read_dir(d0, "")
    assert got == want and len(want) > 20
    # H's and M's sites: files whose rows are theirs alone (each has a size, and so a site, of its own)
    own = 0
    for e in (role["H"], role["M"]):
        r = rows0[rows0[:, 0] == e]
        text = "#thread_rank timestamp offset count\n" + "".join(
            f"{th} {o.t0 + (b << o.bin_shift)} {rw << 12} {c}\n" for _, b, th, rw, c in r.tolist())
        own += sum(1 for s in got.values() if s == text)
    assert own == 2
    # no file holds the stack's row (its offset is past every other object's)
    assert not any(f" {ax.hx.STACK_PAGE << 12} " in s for s in got.values())
    # without the sparse entries' rows those two files are missing
    dense = tx.selected(table, rp.nb_threads, every)
    d1 = str(tmp_path / "dense")
    report_timeline_host(raw, table, d1, rows0[dense[rows0[:, 0]]], **every.kw())
    short = tx.read_dir(d1, "")
    assert len(short) == len(want) - 2 and all(want[n] == s for n, s in short.items())
