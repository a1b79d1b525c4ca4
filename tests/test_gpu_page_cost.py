"""The page cost cells (nmg_set_page_cost): per (object, thread, page) a u64 sum
of 1 or of the weight over the matched samples of chosen memory levels and
accesses, counted on the device beside the page histogram.

Every expectation comes from the oracle (cost_expect.py): the lines of its
all_memory_accesses.dat selected by level string and access and summed per
(entry, thread, page) for the generator's single-bit levels; its per-object
level counters for records with several level bits; its page cells where the
mask selects every record.  The engine's rows must equal them exactly on
attribute_kernel (small tables, NMG_F_SINGLE_PASS) and on every variant of the
partition-first path.

Sizes are test_gpu_timeline.py's: the small case (309 keys) stays on
attribute_kernel, the large one (1509 keys, 60k records) takes two or three
partitions."""
import os

import numpy as np
import pytest

import cost_expect as cx
import placement_expect as px
import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd.replay import MEM_DYNAMIC, T0, ObjectTable, SynthConfig, generate, online_alarms, table_at

pytestmark = pytest.mark.gpu

TINY_POOL = 0x20000    # (internal) private pools of two chunks: the overflow list, overflow_kernel
TINY_OVF = 0x80000     # (internal, with TINY_POOL) an overflow list of 64 records: the rest attributed in the route pass
NO_LINES = 0x20000000  # (internal) route pass without the LDS line stage
VARIANTS = [0, TINY_POOL, TINY_POOL | TINY_OVF, NO_LINES, _lib.NMG_F_SINGLE_PASS]
VARIANT_IDS = ["route", "tinypool", "tinyovf", "nolines", "single"]
LEVELS = _lib.NMG_F_DEFAULT | _lib.NMG_F_OBJECT_LEVELS
STATE, INVALID, CAPACITY = -6, -1, -8

LARGE_CFG = SynthConfig(nb_samples=60_000, nb_intervals=1_500, seed=102)
SMALL_CFG = SynthConfig(nb_samples=20_000, nb_intervals=300, nb_threads=4, seed=101)


class Case:
    """A replay, the oracle's results and dump directory, and the expected rows per option set."""

    def __init__(self, rp, d):
        self.rp = rp
        self.raw, self.odir = cx.run_oracle(rp, d)
        self.dump = cx.Dump(self.odir, rp.table, rp.nb_threads)
        self._rows = {}

    def rows(self, o):
        if o not in self._rows:
            r, n = self.dump.rows(o)
            r.setflags(write=False)
            self._rows[o] = (r, n)
        return self._rows[o][0]

    def nselected(self, o):
        self.rows(o)
        return self._rows[o][1]


COUNT_MEMORY = cx.CostOpts(cx.MEMORY, 3, cx.COUNT)


@pytest.fixture(scope="module")
def small_case(tmp_path_factory):
    c = Case(generate(SMALL_CFG), str(tmp_path_factory.mktemp("cost_small")))
    assert (c.dump.nlines, c.nselected(COUNT_MEMORY), c.rows(COUNT_MEMORY).shape[0], c.dump.unknown) == \
        (16_968, 1_699, 781, 182)
    return c


@pytest.fixture(scope="module")
def large_case(tmp_path_factory):
    c = Case(generate(LARGE_CFG), str(tmp_path_factory.mktemp("cost_large")))
    assert (c.dump.nlines, c.nselected(COUNT_MEMORY), c.rows(COUNT_MEMORY).shape[0], c.dump.unknown) == \
        (50_651, 5_048, 2_297, 495)
    assert c.rp.table.keys.shape[0] > 1023
    return c


def _engine(rp, flags, o, resident=True, **kw):
    """An engine over rp's table with the cost cells set and rp's buffers submitted."""
    import torch
    from numamma_amd.engine import Engine

    eng = Engine(flags=flags, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.set_page_cost(**o.kw(), **kw)
    if resident:
        arena, offs, lens, ranks, acc = rp.packed()
        eng._arena = torch.from_numpy(arena).cuda()  # (the buffers live as long as the engine)
        eng.set_device_buffers(eng._arena.data_ptr(), offs, lens, ranks, acc)
    else:
        eng.submit_replay(rp)
    return eng


def _run(eng):
    eng.analyze()
    eng.synchronize()
    return eng


def _dense_cells(eng, rp):
    """eng.page_cells() of the entries with dense cells, as u64 rows."""
    cells = eng.page_cells()
    return cells[cx.dense(rp.table, rp.nb_threads)[cells[:, 0]]].astype(np.uint64)


def _check(eng, case, o, times=1):
    rows = eng.cost_cells()
    want = case.rows(o).copy()
    want[:, 3] *= np.uint64(times)
    assert rows.dtype == np.uint64 and rows.shape == want.shape and np.array_equal(rows, want)
    return rows


# ---- 1. parity with the oracle's dump, every kernel that attributes

@pytest.mark.parametrize("o", cx.OPTION_SETS, ids=cx.OPTION_IDS)
@pytest.mark.parametrize("resident", [False, True], ids=["staged", "resident"])
def test_small_table(small_case, resident, o):
    eng = _run(_engine(small_case.rp, _lib.NMG_F_DEFAULT, o, resident=resident))
    assert eng.route_count() == 0
    _check(eng, small_case, o)
    eng.close()


@pytest.mark.parametrize("o", cx.OPTION_SETS, ids=cx.OPTION_IDS)
@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
def test_large_table_variants(large_case, extra, o):
    c = large_case
    eng = _run(_engine(c.rp, _lib.NMG_F_DEFAULT | extra, o))
    assert (eng.route_count() == 0) if extra == _lib.NMG_F_SINGLE_PASS else (eng.route_count() > 0)
    rows = _check(eng, c, o)
    if o == cx.EVERYTHING:  # the page cells minus exactly the level-0 lines
        cells = _dense_cells(eng, c.rp)
        assert int(cells[:, 3].sum()) - int(rows[:, 3].sum()) == c.dump.unknown == 495
        key = lambda r: (r[:, 0] << np.uint64(40)) | (r[:, 1] << np.uint64(30)) | r[:, 2]  # noqa: E731
        at = np.searchsorted(key(cells), key(rows))
        assert np.array_equal(key(cells)[at], key(rows)) and (rows[:, 3] <= cells[at, 3]).all()
    eng.close()


# ---- 2. records with several level bits, against the oracle's level counters

@pytest.fixture(scope="module")
def bucket_case(tmp_path_factory):
    rp = generate(LARGE_CFG)
    cx.redraw_levels(rp, 92)
    raw, _ = px.run_oracle(rp, str(tmp_path_factory.mktemp("cost_buckets")))
    lv = cx.oracle_levels(raw)[cx.dense(rp.table, rp.nb_threads)]
    tot = lv.sum(axis=0)  # [2][37]
    assert tot[0].all() and tot[1, 0] and tot[1, 1::2].all()  # every bucket is hit (writes carry weight 0)
    return rp, raw


@pytest.mark.parametrize("extra", [0, TINY_POOL, _lib.NMG_F_SINGLE_PASS], ids=["route", "tinypool", "single"])
@pytest.mark.parametrize("bucket", [5, 11, 17, 18], ids=["remote-ram-hit", "l3-miss", "uncached-miss", "na"])
def test_multi_bit_levels(bucket_case, bucket, extra):
    """One bucket's mask: an entry's rows summed are the oracle's count (COUNT)
    or weight sum (WEIGHT) of that bucket for the entry, per access mask.
    Bucket 5 merges REM_RAM1|2: a record with both bits adds once."""
    rp, raw = bucket_case
    E = rp.table.nb_entries
    ok = cx.dense(rp.table, rp.nb_threads)
    lv = cx.oracle_levels(raw)
    for metric in (cx.COUNT,) if bucket == 18 else (cx.COUNT, cx.WEIGHT):  # (N/A has a count only)
        word = 0 if bucket == 18 else 1 + 2 * bucket + metric
        for access_mask in (1, 2, 3):
            want = np.zeros(E, dtype=np.uint64)
            for a in (0, 1):
                if access_mask & (1 << a):
                    want += lv[:, a, word] * ok.astype(np.uint64)
            if metric == cx.WEIGHT and access_mask == 2:
                assert not want.any()
                continue  # (writes weigh 0: no rows, covered by access_mask 3)
            eng = _run(_engine(rp, _lib.NMG_F_DEFAULT | extra, cx.CostOpts(1 << bucket, access_mask, metric)))
            rows = eng.cost_cells()
            eng.close()
            assert want.any() and np.array_equal(cx.entry_sums(rows, E), want), (metric, access_mask)


# ---- 3. u64 cells and escaped compact records

def escape_replay():
    """test_gpu_timeline.py's escape_replay: weights at the compact record's
    escape values and up to 2^40, timestamps below the table's tbase."""
    rp = generate(LARGE_CFG)
    rng = np.random.default_rng(93)
    wesc = [w for b in range(11, 17) for w in ((1 << b) - 2, (1 << b) - 1, 1 << b)]
    wbig = [(1 << 23) - 1, 1 << 23, (1 << 23) + 5, 1 << 30, 1 << 40]
    for rec in cx.samples(rp):
        u = rng.random(rec.shape[0])
        esc, big, early = u < 0.01, (u >= 0.01) & (u < 0.012), (u >= 0.012) & (u < 0.02)
        rec["weight"][esc] = rng.choice(np.array(wesc, dtype=np.uint64), int(esc.sum()))
        rec["weight"][big] = rng.choice(np.array(wbig, dtype=np.uint64), int(big.sum()))
        rec["timestamp"][early] = rng.integers(1, T0, int(early.sum()), dtype=np.uint64)  # below tbase
    return rp


@pytest.fixture(scope="module")
def escape_case(tmp_path_factory):
    c = Case(escape_replay(), str(tmp_path_factory.mktemp("cost_esc")))
    r = c.rows(ALL_WEIGHT)
    assert int(r[:, 3].max()) >= 1 << 40 and int((r[:, 3] >= 1 << 32).sum()) >= 5  # cells past 32 bits
    return c


ALL_WEIGHT = cx.CostOpts(cx.ALL, 3, cx.WEIGHT)


@pytest.mark.parametrize("rounds", [None, "64"], ids=["default", "r64"])
@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
def test_escaped_records_and_u64_cells(escape_case, extra, rounds, monkeypatch):
    if rounds is None:
        monkeypatch.delenv("NMG_COST_ROUNDS", raising=False)
    else:  # (weights from 2^23 on stay out of the merged sum)
        monkeypatch.setenv("NMG_COST_ROUNDS", rounds)
    eng = _run(_engine(escape_case.rp, _lib.NMG_F_DEFAULT | extra, ALL_WEIGHT))
    _check(eng, escape_case, ALL_WEIGHT)
    eng.close()


# ---- 4. one hot cell, every bound of the merge rounds

def hot_replay():
    """test_gpu_timeline.py's hot_replay: about 30 % of the records on one page
    of the largest long-lived heap object."""
    rp = generate(LARGE_CFG)
    ent = rp.table.entries
    o = tx.TlOpts()
    lo, hi = o.t0 + (5 << o.bin_shift), o.t0 + (6 << o.bin_shift)
    ok = (ent["mem_type"] == MEM_DYNAMIC) & (ent["alloc_date"] <= lo) & (ent["free_date"] >= hi) & \
         (ent["buffer_size"] >= 3 * cx.PAGE)
    e = int(np.argmax(np.where(ok, ent["buffer_size"], 0)))
    assert ok[e]
    rng = np.random.default_rng(7)
    for b, rec in zip(rp.buffers, cx.samples(rp)):
        if b.thread_rank > 2:
            continue
        pick = np.ones(rec.shape[0], bool) if b.thread_rank < 2 else rng.random(rec.shape[0]) < 0.4
        k = int(pick.sum())
        rec["addr"][pick] = ent["buffer_addr"][e] + np.uint64(2 * cx.PAGE) + rng.integers(0, cx.PAGE, k, dtype=np.uint64)
        rec["timestamp"][pick] = rng.integers(lo, hi, k, dtype=np.uint64)
    return rp, e


@pytest.fixture(scope="module")
def hot_case(tmp_path_factory):
    rp, e = hot_replay()
    c = Case(rp, str(tmp_path_factory.mktemp("cost_hot")))
    r = c.rows(cx.EVERYTHING)
    top = r[np.argmax(r[:, 3])]
    assert top[3] >= 4096 and (top[0], top[2]) == (e, 2)  # full merge groups, many chunks on one cell
    return c


@pytest.mark.parametrize("o", [cx.EVERYTHING, ALL_WEIGHT], ids=["count", "weight"])
@pytest.mark.parametrize("extra", [0, TINY_POOL, _lib.NMG_F_SINGLE_PASS], ids=["route", "tinypool", "single"])
def test_hot_cell(hot_case, extra, o, monkeypatch):
    """Whole waves on one cell and many chunks adding to it: the rows are the
    oracle's, hence equal, under NMG_COST_ROUNDS = 0, 1 and 64 (read when the
    cells are set; 64 merges every group) and under the default."""
    for rounds in (None, "0", "1", "64"):
        if rounds is None:
            monkeypatch.delenv("NMG_COST_ROUNDS", raising=False)
        else:
            monkeypatch.setenv("NMG_COST_ROUNDS", rounds)
        eng = _run(_engine(hot_case.rp, _lib.NMG_F_DEFAULT | extra, o))
        _check(eng, hot_case, o)
        eng.close()


# ---- 5. life cycle

def test_accumulate_reset_and_drop(large_case):
    c, o = large_case, cx.MEMORY_WEIGHT
    eng = _engine(c.rp, _lib.NMG_F_DEFAULT, o)
    eng.analyze()
    eng.analyze()
    eng.synchronize()
    _run(eng)
    _check(eng, c, o, times=3)
    eng.reset()
    assert eng.cost_cells().shape == (0, 4)
    _run(eng)
    _check(eng, c, o)
    eng.set_page_cost(cx.REMOTE, 1, cx.COUNT)  # other options: fresh cells
    assert eng.cost_cells().shape == (0, 4)
    _run(eng)
    _check(eng, c, cx.REMOTE_READS)
    eng.set_page_cost(None)
    for getter in (eng.cost_cells, lambda: eng.report_page_cost("/nonexistent"),
                   lambda: eng.object_blocks(2, source=_lib.NMG_PLACE_PAGE_COST)):
        with pytest.raises(_lib.NmgError) as ei:
            getter()
        assert ei.value.code == STATE
    _run(eng)  # (and the kernels run without the cells again)
    eng.set_page_cost(**o.kw())
    eng.set_objects(c.rp.table)  # drops the cells
    with pytest.raises(_lib.NmgError) as ei:
        eng.cost_cells()
    assert ei.value.code == STATE
    assert _lib.lib.nmg_count_cost_cells(eng.h) == STATE
    eng.close()


@pytest.mark.parametrize("extra", [0, _lib.NMG_F_SINGLE_PASS], ids=["route", "single"])
def test_beside_timeline_and_levels(large_case, extra):
    """The extras block with the level rows, the timeline and the cost cells at once."""
    c, o, t = large_case, cx.MEMORY_WEIGHT, tx.TlOpts()
    eng = _engine(c.rp, LEVELS | extra, o, resident=False)
    eng.set_timeline(**t.kw())
    _run(eng)
    assert (eng.route_count() > 0) == (extra == 0)
    _check(eng, c, o)
    want_tl, _ = tx.expected_rows(c.odir, c.rp.table, c.rp.nb_threads, t)
    assert np.array_equal(eng.timeline_cells(), want_tl)
    assert np.array_equal(eng.object_levels(), cx.oracle_levels(c.raw))
    assert np.array_equal(eng.page_cells(), c.raw.cells)
    eng.close()


# ---- 6. streamed chunks

def test_streamed_chunks(large_case):
    from numamma_amd.engine import Engine

    rp, o = large_case.rp, cx.MEMORY_WEIGHT
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.set_page_cost(**o.kw())
    eng.stream_begin(chunk_bytes=640 << 10)  # 2.4 MB of records: four chunks
    for r, a, data in rp.linear_buffers():
        eng.submit_buffer(data, r, a)
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    assert eng.route_count() >= 3
    _check(eng, large_case, o)
    eng.close()


# ---- 7. online: every record selected, so the cost cells are the page cells

def _ent_objs(ent4):
    objs = np.zeros(ent4.shape[0], dtype=[("a", "<u8"), ("s", "<u8"), ("al", "<u8"), ("fr", "<u8")])
    objs["a"], objs["s"], objs["al"], objs["fr"] = ent4[:, 0], ent4[:, 1], ent4[:, 2], ent4[:, 3]
    return objs


def _online_replay(cfg):
    """A replay in online order whose records all carry a non-zero single level
    (the generator's 1 % of level 0 rewritten to an L1 hit)."""
    rp = generate(cfg)
    rp.buffers.reverse()  # online: oldest ring first
    n = 0
    for rec in cx.samples(rp):
        zero = ((rec["data_src"] >> np.uint64(5)) & np.uint64(0x3FFF)) == 0
        rec["data_src"][zero] |= np.uint64((cx.LVL_HIT | cx.LVL_L1) << 5)
        n += int(zero.sum())
    assert n > 0
    return rp


def _cost_equals_page_cells(eng, rp_dense=None):
    rows, cells = eng.cost_cells(), eng.page_cells().astype(np.uint64)
    if rp_dense is not None:
        cells = cells[rp_dense[cells[:, 0]]]
    assert rows.shape[0] > 1000 and np.array_equal(rows, cells)
    return rows


def test_recorded_online_run():
    """nmg_set_objects with the final table, the cost cells, then alarm tables
    listing subsets of its ids (test_gpu_online.py's recorded case).  The page
    cells are pinned to the oracle by that suite; with every record selected
    and counted the cost cells must equal them cell for cell."""
    from numamma_amd.engine import Engine

    rp = _online_replay(SynthConfig(nb_samples=120_000, nb_intervals=2_000, nb_threads=4, with_stack=False,
                                    reuse_frac=0.2, buffer_records=500, seed=72))
    t = rp.table
    snaps = [(be,) + table_at(t, ts) for be, ts in online_alarms(rp, 5)]
    assert snaps[-1][1].shape[0] > 1023 and snaps[0][3].shape[0] < t.nb_entries
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    eng.set_objects(t)
    eng.set_page_cost(**cx.EVERYTHING.kw())
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
    assert eng.route_count() > 0 and eng.global_counters()[2] > 0
    _cost_equals_page_cells(eng, cx.dense(t, rp.nb_threads))
    eng.close()


LIVE_CASES = [
    (SynthConfig(nb_samples=150_000, nb_intervals=600, nb_threads=4, with_stack=False, reuse_frac=0.3,
                 buffer_records=300, seed=81), 7, 1 << 20),
    # the large-table lookup and the partition-first path over an id map
    (SynthConfig(nb_samples=200_000, nb_intervals=20_000, nb_threads=8, with_stack=False, reuse_frac=0.2,
                 realloc_frac=0.05, buffer_records=800, seed=82), 8, 512 << 10),
]


@pytest.mark.parametrize("cfg,nb_alarms,chunk", LIVE_CASES, ids=["k600", "k20k"])
def test_live_online_tables(cfg, nb_alarms, chunk):
    """A live host (test_gpu_online.py's live case): the engine starts from an
    empty table, each alarm's table brings new ids and objects that outgrew
    their cells (every third object is half its final size until it is
    freed), so grow_entries re-lays the cost cells out with the histogram and
    moves grown entries' cells.  Cost cells equal page cells throughout."""
    from numamma_amd.engine import Engine, table_objects

    rp = _online_replay(cfg)
    final = rp.table
    grows = (np.arange(final.nb_entries) % 3) == 0
    snaps, moved = [], 0
    for be, t in online_alarms(rp, nb_alarms):
        keys, off, ids, ent4 = table_at(final, t)
        ent4 = ent4.copy()
        live = (ent4[:, 3] == 0) & grows[ids]
        moved += int((ent4[live, 1] // 2 // 4096 != ent4[live, 1] // 4096).sum())
        ent4[live, 1] = ent4[live, 1] // 2  # size before ma_record_free
        snaps.append((be, keys, off, ids, ent4))
    assert moved > 0  # entries whose page count grows at a later alarm
    ent = final.entries
    order = np.lexsort((np.arange(final.nb_entries), ent["alloc_date"]))
    cid = np.empty(final.nb_entries, dtype=np.uint32)  # live ids: creation order
    cid[order] = np.arange(final.nb_entries, dtype=np.uint32)

    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    eng.set_objects(ObjectTable.empty())  # no objects yet: no cell either
    eng.set_page_cost(**cx.EVERYTHING.kw())
    eng.stream_begin(chunk_bytes=chunk, copy_threads=2)
    b0 = 0
    for k, (be, keys, off, ids, ent4) in enumerate(snaps):
        eng.update_objects(keys, off, cid[ids], _ent_objs(ent4))
        for b in rp.buffers[b0:be]:
            eng.submit_ring(b.ring, b.data_tail, b.data_head, b.thread_rank, b.access_type)
        b0 = be
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    if cfg.nb_intervals > 10_000:
        assert eng.route_count() > 0
    eng.update_objects(final.keys, final.entry_off, cid, table_objects(final))  # ma_finalize's table
    assert eng.global_counters()[2] > 0
    _cost_equals_page_cells(eng)
    eng.close()


# ---- 8. placement from the cost cells

PLACE = [px.Opts(2), px.Opts(4, density_threshold=0), px.Opts(3, thread_node=(2, 0, 1, 1, 0, 2, 2, 1), density_threshold=40)]


@pytest.mark.parametrize("extra", [0, _lib.NMG_F_SINGLE_PASS], ids=["route", "single"])
def test_placement_from_cost(tmp_path, large_case, extra):
    c, o = large_case, cx.MEMORY_WEIGHT
    rp, T = c.rp, c.rp.nb_threads
    eng = _run(_engine(rp, _lib.NMG_F_DEFAULT | extra, o))
    rows = _check(eng, c, o)
    mats = cx.site_matrices(c.odir, T, o)
    for i, po in enumerate(PLACE):
        want = cx.object_blocks(rows, rp.table, T, po)
        assert want.shape[0] > 50
        got = eng.object_blocks(**po.kw(), source=_lib.NMG_PLACE_PAGE_COST)
        assert got.dtype == np.uint64 and np.array_equal(got, want), po
        # the count source is what it was, with cost cells set (and the cache is keyed by the source)
        counts = eng.object_blocks(**po.kw())
        assert np.array_equal(counts, px.object_rows(c.raw, rp.table, po)) and not np.array_equal(counts, want)
        assert np.array_equal(eng.object_blocks(**po.kw(), source=_lib.NMG_PLACE_PAGE_COST), want)
        d = str(tmp_path / f"cost{i}")
        eng.report_placement(d, **po.kw(), source=_lib.NMG_PLACE_PAGE_COST)
        text = cx.site_blocks_text(c.odir, rp.table, mats, po)
        assert text.count("begin_block") > 5 and open(os.path.join(d, "blocks.dat")).read() == text
        d0 = str(tmp_path / f"count{i}")
        eng.report_placement(d0, **po.kw())
        assert open(os.path.join(d0, "blocks.dat")).read() == px.expected_file(c.odir, rp.table, po)
    eng.close()


# ---- 9. the per-site files

@pytest.mark.parametrize("o", [cx.MEMORY_WEIGHT, cx.EVERYTHING], ids=["memory-weight", "all-count"])
def test_report_page_cost(tmp_path, large_case, o):
    c = large_case
    want = cx.site_files(cx.site_matrices(c.odir, c.rp.nb_threads, o))
    assert len(want) > 50
    eng = _run(_engine(c.rp, _lib.NMG_F_DEFAULT, o, resident=False))
    d = str(tmp_path / "out")
    eng.report(d, str(tmp_path / "e.txt"))
    before = cx.read_dir(d, "")
    eng.report_page_cost(d)
    eng.close()
    after = cx.read_dir(d, "")
    assert cx.read_dir(d, "callsite_cost_") == want  # names and bytes
    assert {n: s for n, s in after.items() if not n.startswith("callsite_cost_")} == before
    ids = {int(n[len("callsite_cost_"):-4]) for n in want}
    assert ids <= {sid for sid, _, _ in px.read_sites(c.odir)}  # call_sites.log's ids
    assert px.read_sites(d) == px.read_sites(c.odir)


# ---- 10. errors: the code, and nothing changed after a refused call

def test_rejections(small_case):
    from numamma_amd.engine import Engine, table_objects

    c, o = small_case, cx.MEMORY_WEIGHT
    rp, kw = c.rp, cx.MEMORY_WEIGHT.kw()

    def code(fn):
        with pytest.raises(_lib.NmgError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    assert _lib.lib.nmg_set_page_cost(None, None) == INVALID
    assert _lib.lib.nmg_count_cost_cells(None) == INVALID
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    assert code(lambda: eng.set_page_cost(**kw))[0] == STATE  # before nmg_set_objects
    eng.set_objects(rp.table)
    assert code(eng.cost_cells)[0] == STATE  # no cells set
    assert _lib.lib.nmg_count_cost_cells(eng.h) == STATE
    assert code(lambda: eng.object_blocks(2, source=_lib.NMG_PLACE_PAGE_COST))[0] == STATE
    assert code(lambda: eng.report_placement("/nonexistent", 2, source=_lib.NMG_PLACE_PAGE_COST))[0] == STATE
    pages = rp.table.entries["buffer_size"].astype(np.int64) // 4096 + 1
    need = ((int(pages[cx.dense(rp.table, rp.nb_threads)].sum()) + 3) & ~3) * rp.nb_threads * 8
    eng.set_page_cost(**kw, budget_bytes=need)  # the budget itself
    eng.submit_replay(rp)
    _run(eng)
    _check(eng, c, o)
    for bad in (dict(bucket_mask=0), dict(bucket_mask=1 << 19), dict(access_mask=0), dict(access_mask=4),
                dict(metric=2), dict(reserved=1)):
        assert code(lambda: eng.set_page_cost(**{**kw, **bad}))[0] == INVALID, bad
    rc, msg = code(lambda: eng.set_page_cost(**kw, budget_bytes=need - 1))
    assert rc == CAPACITY and str(need) in msg  # the bytes needed
    for source in (1, 3, 1 << 32):
        assert code(lambda: eng.object_blocks(2, source=source))[0] == INVALID, source
    eng.clear_buffers()
    eng.stream_begin()
    assert code(lambda: eng.set_page_cost(**kw))[0] == STATE  # a stream is open
    eng.stream_end()
    # an update that grows the layout past the cells' budget: refused, nothing changed
    t = rp.table
    big = table_objects(t).copy()
    big["s"][5] += 1 << 20
    rc, msg = code(lambda: eng.update_objects(t.keys, t.entry_off, np.arange(t.nb_entries, dtype=np.uint32), big))
    assert rc == CAPACITY and "page cost" in msg
    _check(eng, c, o)  # the refused calls left the cells and their options alone
    eng.reset()
    eng.clear_buffers()
    eng.submit_replay(rp)
    _run(eng)
    _check(eng, c, o)
    assert np.array_equal(eng.page_cells(), c.raw.cells)
    eng.set_page_cost((1 << 19) - 1, 3, cx.WEIGHT)  # the limits themselves
    eng.close()
    for flags in (_lib.NMG_F_MATCH_SAMPLES, _lib.NMG_F_PAGE_HIST):
        e2 = Engine(flags=flags, nb_threads=rp.nb_threads)
        e2.set_objects(rp.table)
        assert code(lambda: e2.set_page_cost(**kw))[0] == INVALID
        e2.close()
    multi = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, devices=[0, 0])
    multi.set_objects(rp.table)
    assert code(lambda: multi.set_page_cost(**kw))[0] == INVALID
    multi.close()
