"""The access timeline (nmg_set_timeline): per selected object, u32 counters
[time bin][thread][row] of its matched samples, counted on the device.

Every expectation comes from the oracle's dump files, binned in numpy
(timeline_expect.py): all_memory_accesses.dat lists every matched non-stack
sample with thread, timestamp, object id and offset.  The engine's rows must
equal the binned lines exactly, on attribute_kernel (small tables,
NMG_F_SINGLE_PASS) and on every variant of the partition-first path, and the
rows summed over the bins must equal the page cells of the selected entries
grouped by row (the clamp puts every matched sample into exactly one bin).

All cases use t0 = T0 + 2^31, 2^29 ns bins, 12 bins over the generator's
10 s horizon: every bin is used, the first and last collect the clamped
samples.  Sizes: the small case (309 keys) stays on attribute_kernel, the
large one (1509 keys, 60k records) takes two or three partitions."""
import os

import numpy as np
import pytest

import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd.replay import MEM_DYNAMIC, RECORD_DTYPE, T0, SynthConfig, generate, online_alarms, table_at

pytestmark = pytest.mark.gpu

TINY_POOL = 0x20000    # (internal) private pools of two chunks: the overflow list, overflow_kernel
TINY_OVF = 0x80000     # (internal, with TINY_POOL) an overflow list of 64 records: the rest attributed in the route pass
NO_LINES = 0x20000000  # (internal) route pass without the LDS line stage
VARIANTS = [0, TINY_POOL, TINY_POOL | TINY_OVF, NO_LINES, _lib.NMG_F_SINGLE_PASS]
VARIANT_IDS = ["route", "tinypool", "tinyovf", "nolines", "single"]
DUMPS = _lib.NMG_F_DEFAULT | _lib.NMG_F_OBJECT_LEVELS | _lib.NMG_F_SAMPLE_MATCHES
OPTS = tx.TlOpts()
COARSE = tx.TlOpts(min_object_bytes=65536, row_shift=2)


class Case:
    """A replay, the oracle's results and dump directory, and the expected rows per option set."""

    def __init__(self, rp, d):
        self.rp = rp
        self.raw, self.odir = tx.run_oracle(rp, d)
        self._rows = {}

    def rows(self, o=OPTS):
        if o not in self._rows:
            r, n = tx.expected_rows(self.odir, self.rp.table, self.rp.nb_threads, o)
            r.setflags(write=False)
            self._rows[o] = (r, n)
        return self._rows[o][0]

    def nlines(self, o=OPTS):
        self.rows(o)
        return self._rows[o][1]

    def nselected(self, o=OPTS):
        return int(tx.selected(self.rp.table, self.rp.nb_threads, o).sum())


def _all_bins(rows, o=OPTS):
    return set(np.unique(rows[:, 1]).tolist()) == set(range(o.nb_bins))


def _samples(rp):
    return [b.ring.view(RECORD_DTYPE) for b in rp.buffers]


LARGE_CFG = SynthConfig(nb_samples=60_000, nb_intervals=1_500, seed=102)


@pytest.fixture(scope="module")
def small_case(tmp_path_factory):
    c = Case(generate(SynthConfig(nb_samples=20_000, nb_intervals=300, nb_threads=4, seed=101)),
             str(tmp_path_factory.mktemp("tl_small")))
    assert (c.nlines(), c.nselected(), c.rows().shape[0]) == (16_968, 188, 5_422) and _all_bins(c.rows())
    return c


@pytest.fixture(scope="module")
def large_case(tmp_path_factory):
    c = Case(generate(LARGE_CFG), str(tmp_path_factory.mktemp("tl_large")))
    assert (c.nlines(), c.nselected(), c.rows().shape[0]) == (50_651, 721, 12_989) and _all_bins(c.rows())
    assert (c.nselected(COARSE), c.rows(COARSE).shape[0]) == (190, 3_063) and _all_bins(c.rows(COARSE), COARSE)
    assert c.rp.table.keys.shape[0] > 1023
    return c


def hot_replay():
    """The large case with the records of threads 0 and 1, and 40 % of thread
    2's (about 30 % of all), rewritten to one page of the largest heap object
    alive over a whole bin, their timestamps inside that bin."""
    rp = generate(LARGE_CFG)
    ent = rp.table.entries
    lo, hi = OPTS.t0 + (5 << OPTS.bin_shift), OPTS.t0 + (6 << OPTS.bin_shift)
    ok = (ent["mem_type"] == MEM_DYNAMIC) & (ent["alloc_date"] <= lo) & (ent["free_date"] >= hi) & \
         (ent["buffer_size"] >= 3 * tx.PAGE)
    e = int(np.argmax(np.where(ok, ent["buffer_size"], 0)))
    assert ok[e]
    rng = np.random.default_rng(7)
    n = 0
    for b, rec in zip(rp.buffers, _samples(rp)):
        if b.thread_rank > 2:
            continue
        pick = np.ones(rec.shape[0], bool) if b.thread_rank < 2 else rng.random(rec.shape[0]) < 0.4
        k = int(pick.sum())
        rec["addr"][pick] = ent["buffer_addr"][e] + np.uint64(2 * tx.PAGE) + rng.integers(0, tx.PAGE, k, dtype=np.uint64)
        rec["timestamp"][pick] = rng.integers(lo, hi, k, dtype=np.uint64)
        n += k
    total = sum(r.shape[0] for r in _samples(rp))
    assert 0.25 < n / total < 0.35
    return rp, e


@pytest.fixture(scope="module")
def hot_case(tmp_path_factory):
    rp, e = hot_replay()
    c = Case(rp, str(tmp_path_factory.mktemp("tl_hot")))
    r = c.rows()
    top = r[np.argmax(r[:, 4])]
    assert top[4] >= 4096 and (top[0], top[1], top[3]) == (e, 5, 2)  # full merge groups, many chunks on one cell
    return c


def escape_replay():
    """The large case with weights at the compact record's escape values and
    timestamps below the table's tbase (as test_gpu_route_levels.py's
    escape_case), the early ones aimed at objects alive from before T0 or not."""
    rp = generate(LARGE_CFG)
    rng = np.random.default_rng(93)
    wesc = [w for b in range(11, 17) for w in ((1 << b) - 2, (1 << b) - 1, 1 << b)]
    wbig = [(1 << 23) - 1, 1 << 23, (1 << 23) + 5, 1 << 30, 1 << 40]
    nesc = nearly = 0
    for rec in _samples(rp):
        u = rng.random(rec.shape[0])
        esc, big, early = u < 0.01, (u >= 0.01) & (u < 0.012), (u >= 0.012) & (u < 0.02)
        rec["weight"][esc] = rng.choice(np.array(wesc, dtype=np.uint64), int(esc.sum()))
        rec["weight"][big] = rng.choice(np.array(wbig, dtype=np.uint64), int(big.sum()))
        rec["timestamp"][early] = rng.integers(1, T0, int(early.sum()), dtype=np.uint64)  # below tbase
        nesc, nearly = nesc + int(esc.sum()), nearly + int(early.sum())
    assert nesc > 300 and nearly > 300
    return rp


@pytest.fixture(scope="module")
def escape_case(tmp_path_factory):
    c = Case(escape_replay(), str(tmp_path_factory.mktemp("tl_esc")))
    lines = tx._columns(os.path.join(c.odir, "all_memory_accesses.dat"), 2)
    assert int((lines[:, 1] < T0).sum()) > 0  # matched samples from before t0: bin 0
    return c


# ---- running the engine

def _engine(rp, flags, o=OPTS, resident=False, **kw):
    """An engine over rp's table with the timeline set and rp's buffers submitted."""
    import torch
    from numamma_amd.engine import Engine

    eng = Engine(flags=flags, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.set_timeline(**o.kw(), **kw)
    if resident:
        arena, offs, lens, ranks, acc = rp.packed()
        eng._arena = torch.from_numpy(arena).cuda()  # (the buffers live as long as the engine)
        eng.set_device_buffers(eng._arena.data_ptr(), offs, lens, ranks, acc)
    else:
        eng.submit_replay(rp)
    return eng


def _check(eng, case, o=OPTS, times=1):
    """The rows against the oracle-derived ones, and the invariant: the rows
    summed over the bins are the selected entries' page cells grouped by row."""
    rows = eng.timeline_cells()
    want = case.rows(o).copy()
    want[:, 4] *= times
    assert rows.shape == want.shape and np.array_equal(rows, want)
    _check_invariant(eng, case.rp, rows, o)


def _check_invariant(eng, rp, rows, o=OPTS):
    sel = tx.selected(rp.table, rp.nb_threads, o)
    assert np.array_equal(tx.sum_over_bins(rows), tx.page_cells_by_row(eng.page_cells(), sel, o.row_shift))


# ---- 1. small table: attribute_kernel

@pytest.mark.parametrize("resident", [False, True], ids=["staged", "resident"])
def test_small_table(small_case, resident):
    eng = _engine(small_case.rp, _lib.NMG_F_DEFAULT, resident=resident)
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() == 0
    _check(eng, small_case)
    eng.close()


# ---- 2. large table: every route variant, and the single-pass kernel

@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
def test_large_table_variants(large_case, extra):
    eng = _engine(large_case.rp, _lib.NMG_F_DEFAULT | extra, resident=True)
    eng.analyze()
    eng.synchronize()
    assert (eng.route_count() == 0) if extra == _lib.NMG_F_SINGLE_PASS else (eng.route_count() > 0)
    _check(eng, large_case)
    eng.close()


def test_large_table_coarse_rows(large_case):
    eng = _engine(large_case.rp, _lib.NMG_F_DEFAULT, COARSE, resident=True)
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() > 0
    _check(eng, large_case, COARSE)
    eng.close()


# ---- 3. the extras block with all three outputs

@pytest.mark.parametrize("extra", [0, _lib.NMG_F_SINGLE_PASS], ids=["route", "single"])
def test_with_levels_and_sample_matches(large_case, extra):
    eng = _engine(large_case.rp, DUMPS | extra)
    eng.analyze()
    eng.synchronize()
    assert (eng.route_count() > 0) == (extra == 0)
    _check(eng, large_case)
    ent = large_case.raw.entries  # (the oracle's levels as object_levels() lays them out)
    assert np.array_equal(eng.object_levels(), np.stack([ent[:, 3:40], ent[:, 42:79]], axis=1))
    eng.close()


# ---- 4. one hot cell

@pytest.mark.parametrize("rounds", [None, "1", "4", "64"], ids=["default", "r1", "r4", "r64"])
@pytest.mark.parametrize("extra", [0, TINY_POOL, _lib.NMG_F_SINGLE_PASS], ids=["route", "tinypool", "single"])
def test_hot_cell(hot_case, extra, rounds, monkeypatch):
    """7500 records on one cell: whole waves of one cell (one merge group of 64
    lanes) and many chunks adding to it, at every bound of the merge rounds
    (NMG_TL_ROUNDS, read when the timeline is set; 64 merges every group)."""
    if rounds is None:
        monkeypatch.delenv("NMG_TL_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("NMG_TL_ROUNDS", rounds)
    eng = _engine(hot_case.rp, _lib.NMG_F_DEFAULT | extra, resident=True)
    eng.analyze()
    eng.synchronize()
    _check(eng, hot_case)
    eng.close()


# ---- 5. escaped compact records

@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
def test_escaped_records(escape_case, extra):
    c = escape_case
    assert c.rows().shape[0] > 10_000 and _all_bins(c.rows())
    eng = _engine(c.rp, _lib.NMG_F_DEFAULT | extra, resident=True)
    eng.analyze()
    eng.synchronize()
    _check(eng, c)
    eng.close()


# ---- 7. accumulation and reset

def test_accumulate_and_reset(large_case):
    eng = _engine(large_case.rp, _lib.NMG_F_DEFAULT, resident=True)
    eng.analyze()
    eng.analyze()
    eng.synchronize()
    eng.analyze()
    eng.synchronize()
    _check(eng, large_case, times=3)
    eng.reset()
    eng.analyze()
    eng.synchronize()
    _check(eng, large_case)
    eng.set_timeline(None)
    for getter in (eng.timeline_cells, lambda: eng.report_timeline("/nonexistent")):
        with pytest.raises(_lib.NmgError) as ei:
            getter()
        assert ei.value.code == -6  # NMG_ERR_STATE
    eng.analyze()  # (and the kernels run without it again)
    eng.synchronize()
    eng.close()


# ---- 8. streamed chunks

def test_streamed_chunks(large_case):
    from numamma_amd.engine import Engine

    rp = large_case.rp
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.set_timeline(**OPTS.kw())
    eng.stream_begin(chunk_bytes=2 << 20)
    for r, a, data in rp.linear_buffers():
        eng.submit_buffer(data, r, a)
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    assert eng.route_count() >= 2
    _check(eng, large_case)
    eng.close()


# ---- 9. a recorded online run

def _ent_objs(ent4):
    objs = np.zeros(ent4.shape[0], dtype=[("a", "<u8"), ("s", "<u8"), ("al", "<u8"), ("fr", "<u8")])
    objs["a"], objs["s"], objs["al"], objs["fr"] = ent4[:, 0], ent4[:, 1], ent4[:, 2], ent4[:, 3]
    return objs


def test_recorded_online_run():
    """nmg_set_objects with the final table, the timeline, then alarm tables
    listing subsets of its ids (test_gpu_online.py's recorded case).  The
    oracle writes no dumps in alarm mode: the invariant against page_cells()
    is the check.  An update the layout cannot follow is refused whole."""
    from numamma_amd.engine import Engine, table_objects

    rp = generate(SynthConfig(nb_samples=120_000, nb_intervals=2_000, nb_threads=4, with_stack=False, reuse_frac=0.2,
                              buffer_records=500, seed=72))
    rp.buffers.reverse()  # online: oldest ring first
    t = rp.table
    snaps = [(be,) + table_at(t, ts) for be, ts in online_alarms(rp, 5)]
    assert snaps[-1][1].shape[0] > 1023 and snaps[0][3].shape[0] < t.nb_entries
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    eng.set_objects(t)
    eng.set_timeline(**OPTS.kw())

    def run():
        eng.stream_begin(chunk_bytes=256 << 10, copy_threads=2)
        b0 = 0
        for be, keys, off, ids, ent4 in snaps:
            eng.update_objects(keys, off, ids, _ent_objs(ent4))
            for b in rp.buffers[b0:be]:
                eng.submit_ring(b.ring, b.data_tail, b.data_head, b.thread_rank, b.access_type)
            b0 = be
        eng.analyze()
        eng.stream_end()
        eng.synchronize()
        rows = eng.timeline_cells()
        assert rows.shape[0] > 0 and eng.global_counters()[2] > 0  # (objects freed before an alarm did match)
        _check_invariant(eng, rp, rows)
        return rows

    first = run()
    assert eng.route_count() > 0
    # a new id, and a listed entry with another size: refused, nothing changed
    _, keys, off, ids, ent4 = snaps[-1]
    grown = _ent_objs(ent4)
    grown["s"][3] += 4096
    with pytest.raises(_lib.NmgError) as ei:
        eng.update_objects(keys, off, ids, grown)
    assert ei.value.code == -6
    more = np.concatenate([ids[:-1], np.array([t.nb_entries], dtype=np.uint32)])
    with pytest.raises(_lib.NmgError) as ei:
        eng.update_objects(keys, off, more, _ent_objs(ent4))
    assert ei.value.code == -6
    eng.nb_entries = t.nb_entries  # (the binding counted the refused id)
    eng.reset()
    eng.clear_buffers()
    assert np.array_equal(run(), first)
    eng.update_objects(t.keys, t.entry_off, np.arange(t.nb_entries, dtype=np.uint32), table_objects(t))
    eng.close()


# ---- 10. errors

def test_rejections(small_case):
    from numamma_amd.engine import Engine

    rp = small_case.rp
    kw = OPTS.kw()

    def code(fn):
        with pytest.raises(_lib.NmgError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    assert _lib.lib.nmg_set_timeline(None, None) == -1
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    assert code(lambda: eng.set_timeline(**kw))[0] == -6  # before nmg_set_objects
    eng.set_objects(rp.table)
    assert code(eng.timeline_cells)[0] == -6  # no timeline set
    assert _lib.lib.nmg_count_timeline_cells(eng.h) == -6
    for bad in (dict(bin_shift=64), dict(nb_bins=0), dict(nb_bins=4097), dict(row_shift=21), dict(reserved=1)):
        assert code(lambda: eng.set_timeline(**{**kw, **bad}))[0] == -1, bad
    c, msg = code(lambda: eng.set_timeline(**kw, budget_bytes=700_000))
    assert c == -8 and "705984" in msg  # the bytes needed (188 entries' cells)
    eng.set_timeline(**kw, budget_bytes=705_984)
    eng.set_timeline(**{**kw, "nb_bins": 4096, "bin_shift": 63, "row_shift": 20})  # the limits themselves
    eng.stream_begin()
    assert code(lambda: eng.set_timeline(**kw))[0] == -6  # a stream is open
    eng.stream_end()
    eng.set_objects(rp.table)  # drops the timeline
    assert code(eng.timeline_cells)[0] == -6
    eng.close()
    for flags in (_lib.NMG_F_MATCH_SAMPLES, _lib.NMG_F_PAGE_HIST):
        e2 = Engine(flags=flags, nb_threads=rp.nb_threads)
        e2.set_objects(rp.table)
        assert code(lambda: e2.set_timeline(**kw))[0] == -1
        e2.close()
    multi = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, devices=[0, 0])
    multi.set_objects(rp.table)
    assert code(lambda: multi.set_timeline(**kw))[0] == -1
    multi.close()


# ---- 11. the per-site files

def test_report_timeline(tmp_path, large_case):
    c = large_case
    o = tx.TlOpts(min_object_bytes=0)  # every non-stack entry
    want = tx.expected_site_files(c.odir, o)
    assert len(want) > 50 and c.nselected(o) > c.nselected()
    eng = _engine(c.rp, _lib.NMG_F_DEFAULT, o)
    eng.analyze()
    eng.synchronize()
    _check(eng, c, o)
    d = str(tmp_path / "out")
    eng.report(d, str(tmp_path / "e.txt"))
    before = tx.read_dir(d, "")
    eng.report_timeline(d)
    eng.close()
    after = tx.read_dir(d, "")
    assert tx.read_dir(d, "callsite_timeline_") == want  # the oracle's per-site dumps, binned; the same ids
    assert {n: s for n, s in after.items() if not n.startswith("callsite_timeline_")} == before
