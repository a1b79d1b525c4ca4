"""nmg_report_timeline_host on the CPU: the oracle's raw results plus timeline
rows binned in numpy from its all_memory_accesses.dat give, per call site, a
callsite_timeline_<id>.dat equal to the oracle's callsite_dump_<id>.dat binned
by the same rule -- the same set of site ids (the registry nmg_report uses),
cells of a site's objects summed, lines in (bin, thread, row) order."""
import os

import numpy as np
import pytest

import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd.replay import SynthConfig, generate
from numamma_amd.results import report_host, report_timeline_host


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    rp = generate(SynthConfig(nb_samples=60_000, nb_intervals=1_500, seed=102))
    raw, odir = tx.run_oracle(rp, str(tmp_path_factory.mktemp("tlhost")))
    return rp, raw, odir


@pytest.mark.parametrize("row_shift", [0, 2])
def test_site_files_match_binned_oracle_dumps(tmp_path, case, row_shift):
    rp, raw, odir = case
    o = tx.TlOpts(min_object_bytes=0, row_shift=row_shift)  # every non-stack entry
    rows, nlines = tx.expected_rows(odir, rp.table, rp.nb_threads, o)
    want = tx.expected_site_files(odir, o)
    # the expectation is not degenerate: many sites, every bin, sites with several objects' cells
    assert nlines > 40_000 and len(want) > 50
    assert set(np.unique(rows[:, 1]).tolist()) == set(range(o.nb_bins))
    assert int(rows[:, 4].sum()) == nlines
    pdir = str(tmp_path / "product")
    report_timeline_host(raw, rp.table, pdir, rows, **o.kw())
    assert tx.read_dir(pdir, "") == want  # (nothing but the timeline files is written)
    # the ids are nmg_report_host's for the same results
    rdir = str(tmp_path / "report")
    report_host(raw, rp.table, np.zeros(raw.nb_buffers, dtype=np.uint64), rdir, str(tmp_path / "p.txt"))
    ids = {n[len("callsite_timeline_"):] for n in want}
    assert ids <= {n[len("callsite_counters_"):] for n in os.listdir(rdir) if n.startswith("callsite_counters_")}


def test_rows_in_any_order_and_split_cells(tmp_path, case):
    """The writer groups by site itself: shuffled rows, and a cell given in two
    parts, give the same files."""
    rp, raw, odir = case
    o = tx.TlOpts(min_object_bytes=0)
    rows, _ = tx.expected_rows(odir, rp.table, rp.nb_threads, o)
    big = rows[rows[:, 4] > 1]
    assert big.shape[0] > 100
    part = big.copy()
    part[:, 4] = 1
    rest = rows.copy()
    rest[rows[:, 4] > 1, 4] -= 1
    mixed = np.concatenate([rest, part])
    mixed = mixed[np.random.default_rng(5).permutation(mixed.shape[0])]
    pdir = str(tmp_path / "product")
    report_timeline_host(raw, rp.table, pdir, mixed, **o.kw())
    assert tx.read_dir(pdir, "") == tx.expected_site_files(odir, o)


def test_host_function_rejects_bad_arguments(case):
    rp, raw, odir = case
    o = tx.TlOpts(min_object_bytes=0)
    rows, _ = tx.expected_rows(odir, rp.table, rp.nb_threads, o)
    assert _lib.lib.nmg_report_timeline_host(None, None, None, None, None, 0) == -1
    for bad in (dict(nb_bins=0), dict(nb_bins=4097), dict(bin_shift=64), dict(row_shift=21), dict(reserved=1)):
        with pytest.raises(_lib.NmgError) as ei:
            report_timeline_host(raw, rp.table, "/nonexistent", rows, **{**o.kw(), **bad})
        assert ei.value.code == -1, bad
    for col, val in ((0, raw.nb_entries), (1, o.nb_bins), (2, rp.nb_threads)):  # entry, bin, thread out of range
        r = rows.copy()
        r[7, col] = val
        with pytest.raises(_lib.NmgError) as ei:
            report_timeline_host(raw, rp.table, "/nonexistent", r, **o.kw())
        assert ei.value.code == -1
