"""Page cost cells of every entry (nmg_set_page_cost_ex, NMG_COST_SCOPE_ALL):
the sparse entries -- [stack], objects past the per-entry cap, whatever the
histogram budget left sparse -- keep a u64 cost beside their page count, at
the count's slot of the sparse page table.

Every expectation comes from the oracle (cost_all_expect.py): the lines of its
-D dump for the non-stack entries, sparse or not; for [stack], which the dump
omits, its per-object level counters (one-bucket masks) and its page cells
(records redrawn from the levels that every-bucket selects).  The rows must be
equal on attribute_kernel (the small table with a truly huge object) and on
every variant of the partition-first path, under every histogram budget."""
import ctypes as C
import os

import numpy as np
import pytest

import cost_all_expect as ax
import cost_expect as cx
import placement_expect as px
import placement_huge_expect as hx
from numamma_amd import _lib
from numamma_amd.replay import RECORD_DTYPE, ObjectTable, SynthConfig, generate, online_alarms, table_at
from test_gpu_placement_huge import ALL_SPARSE, CAP, DEFAULT_BUDGET, _kinds, _mid_budget, dense_model

pytestmark = pytest.mark.gpu

TINY_POOL = 0x20000  # (internal) private pools of two chunks: the overflow list, overflow_kernel
TINY_OVF = 0x80000   # (internal, with TINY_POOL) an overflow list of 64 records: the rest attributed in the route pass
VARIANTS = [0, TINY_POOL, TINY_POOL | TINY_OVF, _lib.NMG_F_SINGLE_PASS]
VARIANT_IDS = ["route", "tinypool", "tinyovf", "single"]
STATE, INVALID, CAPACITY = -6, -1, -8
ALL, DENSE = _lib.NMG_COST_SCOPE_ALL, _lib.NMG_COST_SCOPE_DENSE
COST, HUGE = _lib.NMG_PLACE_PAGE_COST, _lib.NMG_PLACE_HUGE
LARGE_CFG = SynthConfig(nb_samples=60_000, nb_intervals=1_500, seed=102)
BUCKETS = [5, 11, 17, 18]


def _engine(rp, o, budget=0, flags=_lib.NMG_F_DEFAULT, scope=ALL, submit=True, **kw):
    from numamma_amd.engine import Engine

    eng = Engine(flags=flags, nb_threads=rp.nb_threads, hist_budget_bytes=budget, sparse_capacity=CAP)
    eng.set_objects(rp.table)
    eng.set_page_cost(**o.kw(), scope=scope, **kw)
    if submit:
        eng.submit_replay(rp)
    return eng


def _run(eng):
    eng.analyze()
    eng.synchronize()
    return eng


def _u64(cells):
    return cells.astype(np.uint64)


def _eq(got, want):
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)


class Case:
    """A replay, the oracle's results and -D dump over every entry, the expected non-stack rows per option set."""

    def __init__(self, rp, d, role=None):
        self.rp, self.role = rp, role
        self.raw, self.odir = cx.run_oracle(rp, d)
        self.dump = ax.DumpAll(self.odir, rp.table, rp.nb_threads)
        self.st = ax.stack_entry(rp.table)
        self.nstack = ax.check_dump_covers(self.dump, self.raw, rp.table)  # on the CPU, before any engine runs
        self._rows = {}

    def rows(self, o):
        if o not in self._rows:
            r = self.dump.rows(o)[0]
            r.setflags(write=False)
            self._rows[o] = r
        return self._rows[o]

    def check(self, rows, o, times=1):
        """The non-stack rows are the dump's; the stack's lie on its page cells (returned)."""
        mine = rows[:, 0] == self.st
        _eq(rows[~mine], ax.with_times(self.rows(o), times))
        cells = _u64(self.raw.cells)
        sc = cells[cells[:, 0] == self.st]
        key = lambda r: (r[:, 1] << np.uint64(32)) | r[:, 2]  # noqa: E731
        assert np.isin(key(rows[mine]), key(sc)).all()
        if o.metric == cx.COUNT:
            at = np.searchsorted(key(sc), key(rows[mine]))
            assert (rows[mine][:, 3] <= sc[at, 3] * np.uint64(times)).all()
        return rows[mine]


@pytest.fixture(scope="module")
def huge(tmp_path_factory):
    rp, role = hx.huge_replay(stack=True)
    c = Case(rp, str(tmp_path_factory.mktemp("costall_huge")), role)
    cells = c.raw.cells
    assert c.st == role["stack"] and int(cells[cells[:, 0] == c.st][:, 3].sum()) >= 20
    ok = cx.dense(rp.table, rp.nb_threads)
    assert not ok[role["H"]] and not ok[role["M"]]
    want = c.rows(cx.EVERYTHING)[:, 0]
    H, M = role["H"], role["M"]
    assert (want == H).any() and (want == M).any() and (want < M).sum() > 20 and ((want > M) & (want < H)).sum() > 20
    return c


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    c = Case(generate(LARGE_CFG), str(tmp_path_factory.mktemp("costall_large")))
    assert c.rp.table.keys.shape[0] > 1023
    c.mid = _mid_budget(c.rp.table)
    dm = dense_model(c.rp.table, c.rp.nb_threads, c.mid)
    r = c.rows(cx.MEMORY_WEIGHT)[:, 0].astype(np.int64)
    assert dm[r].sum() > 300 and (~dm[r]).sum() > 300  # expected rows of both kinds at the mid budget
    return c


def _redrawn(make, d, seed, levels=None):
    """(replay, raw, stack entry) with every record's level redrawn; the stack entry has at least 20 matched samples."""
    rp = make()
    if levels is None:
        cx.redraw_levels(rp, seed)
    else:
        cx.redraw_levels(rp, seed, levels=levels)
    raw, _ = px.run_oracle(rp, d)
    st = ax.stack_entry(rp.table)
    cells = raw.cells
    assert int(cells[cells[:, 0] == st][:, 3].sum()) >= 20
    return rp, raw, st


# ---- 1. the small table: attribute_kernel, H and M past the per-entry cap, [stack]

@pytest.mark.parametrize("o", cx.OPTION_SETS, ids=cx.OPTION_IDS)
def test_small_table(huge, o):
    c = huge
    eng = _run(_engine(c.rp, o))
    assert eng.route_count() == 0
    rows = eng.cost_cells()
    stack_rows = c.check(rows, o)
    if o == cx.EVERYTHING:
        H, M, ids = c.role["H"], c.role["M"], rows[:, 0]
        assert stack_rows.shape[0] > 0 and (ids == H).any() and (ids == M).any()
        assert (ids < M).sum() > 20 and ((ids > M) & (ids < H)).sum() > 20  # dense entries on both sides of M
        assert ((stack_rows[:, 1] == hx.T_A) & (stack_rows[:, 2] == hx.STACK_PAGE)).any()
    assert np.array_equal(eng.page_cells(), c.raw.cells)
    eng.close()


@pytest.fixture(scope="module")
def huge_cells(tmp_path_factory):
    return _redrawn(lambda: hx.huge_replay(stack=True)[0], str(tmp_path_factory.mktemp("costall_hcells")), 94,
                    levels=ax.SELECTED)


def test_small_table_every_cell(huge_cells):
    """Records redrawn from the selected levels, every bucket, counted: the cost
    rows of every entry, [stack] included, are the oracle's page cells."""
    rp, raw, st = huge_cells
    eng = _run(_engine(rp, cx.EVERYTHING))
    assert eng.route_count() == 0
    rows = eng.cost_cells()
    _eq(rows, _u64(raw.cells))
    assert (rows[:, 0] == st).any()
    eng.close()


@pytest.fixture(scope="module")
def huge_levels(tmp_path_factory):
    rp, raw, st = _redrawn(lambda: hx.huge_replay(stack=True)[0], str(tmp_path_factory.mktemp("costall_hlev")), 92)
    # [stack] has samples in some tested bucket, and the sparse entries in every one
    assert any(ax.bucket_sums(raw, b, cx.COUNT, 3)[st] for b in BUCKETS)
    ok = cx.dense(rp.table, rp.nb_threads)
    assert all(ax.bucket_sums(raw, b, cx.COUNT, 3)[~ok].any() for b in BUCKETS)
    return rp, raw, st


@pytest.mark.parametrize("bucket", BUCKETS, ids=["remote-ram-hit", "l3-miss", "uncached-miss", "na"])
def test_small_table_one_bucket(huge_levels, bucket):
    """test_gpu_page_cost.py's test_multi_bit_levels without its dense filter: an
    entry's rows summed are the oracle's count or weight sum of the bucket."""
    rp, raw, st = huge_levels
    E = rp.table.nb_entries
    for metric in (cx.COUNT,) if bucket == 18 else (cx.COUNT, cx.WEIGHT):
        for access_mask in (1, 2, 3):
            want = ax.bucket_sums(raw, bucket, metric, access_mask)
            if metric == cx.WEIGHT and access_mask == 2:
                assert not want.any()
                continue  # (writes weigh 0: no rows, covered by access_mask 3)
            eng = _run(_engine(rp, cx.CostOpts(1 << bucket, access_mask, metric)))
            rows = eng.cost_cells()
            eng.close()
            assert want.any() and np.array_equal(cx.entry_sums(rows, E), want), (metric, access_mask)


# ---- 2. the partition-first path: local_kernel's extras, overflow_kernel, the route pass, process_sample

def _budget_kinds(eng, c, budget):
    ns, nd = _kinds(eng, c.raw, c.rp.table, budget)
    dm = dense_model(c.rp.table, c.rp.nb_threads, budget or DEFAULT_BUDGET)
    if budget == ALL_SPARSE:
        assert not dm.any() and nd == 0 and ns > 1000
    elif budget == c.mid:
        assert ns > 1000 and nd > 1000
    return dm


@pytest.mark.parametrize("o", cx.OPTION_SETS, ids=cx.OPTION_IDS)
@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("budget", ["one-cell", "mid"])
def test_route_path(large, budget, extra, o):
    c = large
    b = ALL_SPARSE if budget == "one-cell" else c.mid
    eng = _run(_engine(c.rp, o, b, flags=_lib.NMG_F_DEFAULT | extra))
    assert (eng.route_count() == 0) if extra == _lib.NMG_F_SINGLE_PASS else (eng.route_count() > 0)
    _budget_kinds(eng, c, b)
    c.check(eng.cost_cells(), o)
    eng.close()


def _large_with_stack():
    """LARGE_CFG with 24 records of the first buffer aimed at two pages of [stack] (ts = 0, as huge_replay plants them)."""
    rp = generate(LARGE_CFG)
    ent = rp.table.entries
    st = ax.stack_entry(rp.table)
    b = rp.buffers[0]
    rec = b.ring.view(RECORD_DTYPE)
    assert b.data_tail == 0 and rec.shape[0] > 24
    rec["addr"][:24] = int(ent["buffer_addr"][st]) + np.repeat(np.array([3, hx.STACK_PAGE], dtype=np.uint64), 12) * np.uint64(4096)
    rec["timestamp"][:24] = 0
    return rp


@pytest.fixture(scope="module")
def large_cells(tmp_path_factory):
    return _redrawn(_large_with_stack, str(tmp_path_factory.mktemp("costall_lcells")), 95, levels=ax.SELECTED)


@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("budget", ["one-cell", "mid"])
def test_route_path_every_cell(large, large_cells, budget, extra):
    """[stack] on the partition-first path: every record selected and counted, the rows are the page cells."""
    rp, raw, st = large_cells
    eng = _run(_engine(rp, cx.EVERYTHING, ALL_SPARSE if budget == "one-cell" else large.mid,
                       flags=_lib.NMG_F_DEFAULT | extra))
    assert (eng.route_count() == 0) if extra == _lib.NMG_F_SINGLE_PASS else (eng.route_count() > 0)
    rows = eng.cost_cells()
    _eq(rows, _u64(raw.cells))
    assert (rows[:, 0] == st).any()
    eng.close()


# ---- 3. budget invariance

@pytest.mark.parametrize("o", [cx.MEMORY_WEIGHT, cx.EVERYTHING], ids=["memory-weight", "all-count"])
def test_budget_invariance(large, o):
    c = large
    got = []
    for b in (ALL_SPARSE, c.mid, 0):
        eng = _run(_engine(c.rp, o, b))
        got.append(eng.cost_cells())
        eng.close()
    c.check(got[0], o)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


# ---- 4. accumulate and reset

@pytest.mark.parametrize("budget", ["one-cell", "mid"])
def test_accumulate_and_reset(large, budget):
    c, o = large, cx.MEMORY_WEIGHT
    eng = _run(_engine(c.rp, o, ALL_SPARSE if budget == "one-cell" else c.mid))
    once = eng.cost_cells()
    c.check(once, o)
    _run(eng)
    _eq(eng.cost_cells(), ax.with_times(once, 2))
    eng.reset()
    assert eng.cost_cells().shape == (0, 4)  # (a reused slot keeps no old cost)
    _run(eng)
    _eq(eng.cost_cells(), once)
    eng.reset()
    eng.set_page_cost(**cx.REMOTE_READS.kw(), scope=ALL)  # other options: fresh cells
    _run(eng)
    c.check(eng.cost_cells(), cx.REMOTE_READS)
    eng.close()


# ---- 5. streamed chunks and online alarms, at the one-cell budget

def test_streamed_chunks(large):
    from numamma_amd.engine import Engine

    c, o = large, cx.MEMORY_WEIGHT
    rp = c.rp
    batch = _run(_engine(rp, o, ALL_SPARSE))
    want = batch.cost_cells()
    batch.close()
    c.check(want, o)
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=ALL_SPARSE, sparse_capacity=CAP)
    eng.set_objects(rp.table)
    eng.set_page_cost(**o.kw(), scope=ALL)
    eng.stream_begin(chunk_bytes=640 << 10)  # 2.4 MB of records: four chunks
    for r, a, data in rp.linear_buffers():
        eng.submit_buffer(data, r, a)
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    assert eng.route_count() >= 3
    _eq(eng.cost_cells(), want)
    eng.close()


def _ent_objs(ent4):
    objs = np.zeros(ent4.shape[0], dtype=[("a", "<u8"), ("s", "<u8"), ("al", "<u8"), ("fr", "<u8")])
    objs["a"], objs["s"], objs["al"], objs["fr"] = ent4[:, 0], ent4[:, 1], ent4[:, 2], ent4[:, 3]
    return objs


def _online_replay(cfg):
    """Online order, every record with a selected level (test_gpu_page_cost.py's _online_replay)."""
    rp = generate(cfg)
    rp.buffers.reverse()
    for rec in cx.samples(rp):
        zero = ((rec["data_src"] >> np.uint64(5)) & np.uint64(0x3FFF)) == 0
        rec["data_src"][zero] |= np.uint64((cx.LVL_HIT | cx.LVL_L1) << 5)
    return rp


def test_recorded_online_run():
    """The final table, the cells, then alarm tables over subsets of its ids:
    with every record selected and counted the cost rows are the page cells
    (pinned to the oracle by test_gpu_online.py), all of them sparse here."""
    from numamma_amd.engine import Engine

    rp = _online_replay(SynthConfig(nb_samples=60_000, nb_intervals=1_500, nb_threads=4, with_stack=False,
                                    reuse_frac=0.2, buffer_records=500, seed=72))
    t = rp.table
    snaps = [(be,) + table_at(t, ts) for be, ts in online_alarms(rp, 3)]
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=ALL_SPARSE, sparse_capacity=CAP)
    eng.set_objects(t)
    eng.set_page_cost(**cx.EVERYTHING.kw(), scope=ALL)
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
    rows, cells = eng.cost_cells(), _u64(eng.page_cells())
    assert rows.shape[0] > 1000 and eng.sparse_export()[0].shape[0] == rows.shape[0]
    _eq(rows, cells)
    eng.close()


def test_live_online_first_sparse_entry():
    """A live host from an empty table: the first alarm's update brings the
    first sparse entries, so grow_entries allocates the sparse cost cells with
    the sparse page table; later alarms bring more.  Cost rows = page cells."""
    from numamma_amd.engine import Engine, table_objects

    rp = _online_replay(SynthConfig(nb_samples=60_000, nb_intervals=600, nb_threads=4, with_stack=False, reuse_frac=0.3,
                                    buffer_records=300, seed=81))
    final = rp.table
    ent = final.entries
    order = np.lexsort((np.arange(final.nb_entries), ent["alloc_date"]))
    cid = np.empty(final.nb_entries, dtype=np.uint32)  # live ids: creation order
    cid[order] = np.arange(final.nb_entries, dtype=np.uint32)
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=ALL_SPARSE, sparse_capacity=CAP)
    eng.set_objects(ObjectTable.empty())
    # a budget below the sparse array: the update that would bring the sparse table is refused, nothing changed
    eng.set_page_cost(**cx.EVERYTHING.kw(), scope=ALL, budget_bytes=8 * CAP - 1)
    be, t0 = list(online_alarms(rp, 4))[0]
    keys, off, ids, ent4 = table_at(final, t0)
    with pytest.raises(_lib.NmgError) as ei:
        eng.update_objects(keys, off, cid[ids], _ent_objs(ent4))
    assert ei.value.code == CAPACITY and "page cost" in str(ei.value) and str(8 * CAP) in str(ei.value)
    assert eng.cost_cells().shape == (0, 4) and eng.page_cells().shape[0] == 0
    eng.set_page_cost(**cx.EVERYTHING.kw(), scope=ALL, budget_bytes=8 * CAP)
    eng.stream_begin(chunk_bytes=1 << 20, copy_threads=2)
    b0 = 0
    for be, t in online_alarms(rp, 4):
        keys, off, ids, ent4 = table_at(final, t)
        eng.update_objects(keys, off, cid[ids], _ent_objs(ent4))
        for b in rp.buffers[b0:be]:
            eng.submit_ring(b.ring, b.data_tail, b.data_head, b.thread_rank, b.access_type)
        b0 = be
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    eng.update_objects(final.keys, final.entry_off, cid, table_objects(final))
    rows = eng.cost_cells()
    assert rows.shape[0] > 1000 and eng.global_counters()[2] > 0
    _eq(rows, _u64(eng.page_cells()))
    eng.close()


# ---- 6. placement from the cost cells

def test_placement(huge, huge_cells):
    rp, raw, st = huge_cells
    table, T = rp.table, rp.nb_threads
    H, M = huge.role["H"], huge.role["M"]
    o = hx.PRIMARY
    # every cell selected: the expected cost rows are the oracle's page cells, [stack] included
    want = ax.object_blocks_all(_u64(raw.cells), table, T, o)
    assert np.array_equal(want, hx.object_rows_all(raw, table, o))
    for e in (H, M, st):
        assert (want[:, 0] == e).any()
    eng = _run(_engine(rp, cx.EVERYTHING))
    _eq(eng.object_blocks(**o.kw(), source=COST), want)
    _eq(eng.object_blocks(**o.kw(), source=HUGE), want)  # (the counts, here equal)
    with pytest.raises(_lib.NmgError) as ei:
        eng.object_blocks(**o.kw(), source=COST | HUGE)
    assert ei.value.code == INVALID and "sparse entries have no cost cells" in str(ei.value)
    eng.close()
    # the weight metric over the generator's levels: the non-stack entries' blocks from the dump's rows
    c, ow, po = huge, cx.MEMORY_WEIGHT, px.Opts(4, (0, 0, 1, 1, 3, 3, 3, 3), 0)
    eng = _run(_engine(c.rp, ow))
    rows = eng.cost_cells()
    c.check(rows, ow)
    got = eng.object_blocks(**po.kw(), source=COST)
    _eq(got, ax.object_blocks_all(rows, c.rp.table, T, po))
    wantw = ax.object_blocks_all(c.rows(ow), c.rp.table, T, po)
    _eq(got[got[:, 0] != c.st], wantw)
    assert (wantw[:, 0] == H).any() or (wantw[:, 0] == M).any()
    eng.close()
    # the dense scope: today's rows
    eng = _run(_engine(c.rp, ow, scope=DENSE))
    dense_rows = c.dump.dense_rows(ow)
    _eq(eng.cost_cells(), dense_rows)
    gotd = eng.object_blocks(**po.kw(), source=COST)
    _eq(gotd, cx.object_blocks(dense_rows, c.rp.table, T, po))
    assert not np.isin(gotd[:, 0], [H, M, c.st]).any() and gotd.shape[0] < got.shape[0]
    with pytest.raises(_lib.NmgError) as ei:
        eng.object_blocks(**po.kw(), source=COST | HUGE)
    assert ei.value.code == INVALID and "sparse entries have no cost cells" in str(ei.value)
    # the scope is part of what the cached blocks are made for
    eng.set_page_cost(**ow.kw(), scope=ALL)
    _run(eng)
    _eq(eng.object_blocks(**po.kw(), source=COST), got)
    eng.close()


# ---- 7. the per-site files and blocks.dat, sites with a dense and a sparse member

@pytest.mark.parametrize("o", [cx.MEMORY_WEIGHT, cx.EVERYTHING], ids=["memory-weight", "all-count"])
def test_reports(tmp_path, large, o):
    c = large
    table, T = c.rp.table, c.rp.nb_threads
    ent = table.entries
    dm = dense_model(table, T, c.mid)
    site = {}
    for e in range(table.nb_entries):
        if e != c.st:
            site.setdefault((table.caller(e), int(ent["initial_buffer_size"][e])), set()).add(bool(dm[e]))
    assert any(len(v) == 2 for v in site.values())
    mats = cx.site_matrices(c.odir, T, o)
    want = cx.site_files(mats)
    assert len(want) > 50
    eng = _run(_engine(c.rp, o, c.mid))
    _budget_kinds(eng, c, c.mid)
    d = str(tmp_path / "cost")
    eng.report_page_cost(d)
    assert cx.read_dir(d, "") == want
    po = px.Opts(4, density_threshold=0)
    d2 = str(tmp_path / "place")
    eng.report_placement(d2, **po.kw(), source=COST)
    text = cx.site_blocks_text(c.odir, table, mats, po)
    assert text.count("begin_block") > 5 and open(os.path.join(d2, "blocks.dat")).read() == text
    eng.close()


# ---- 8. errors and the budget

def test_errors_and_budget(large):
    c, o = large, cx.MEMORY_WEIGHT
    rp, kw = c.rp, cx.MEMORY_WEIGHT.kw()
    T = rp.nb_threads

    def code(fn):
        with pytest.raises(_lib.NmgError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    pages = rp.table.entries["buffer_size"].astype(np.int64) // 4096 + 1
    dm = dense_model(rp.table, T, c.mid)
    dense_bytes = ((int(pages[dm].sum()) + 3) & ~3) * T * 8
    need = dense_bytes + 8 * CAP
    eng = _engine(rp, o, c.mid, budget_bytes=need)  # the budget itself
    assert code(lambda: eng.set_page_cost(**kw, scope=2))[0] == INVALID
    assert code(lambda: eng.set_page_cost(**kw, scope=1 << 31))[0] == INVALID
    assert code(lambda: eng.set_page_cost(**kw, scope=ALL, reserved=1))[0] == INVALID
    rc, msg = code(lambda: eng.set_page_cost(**kw, scope=ALL, budget_bytes=need - 1))
    assert rc == CAPACITY and str(need) in msg
    eng.set_page_cost(**kw, scope=DENSE, budget_bytes=dense_bytes)  # the dense scope needs the dense array only
    rc, msg = code(lambda: eng.set_page_cost(**kw, scope=DENSE, budget_bytes=dense_bytes - 1))
    assert rc == CAPACITY and str(dense_bytes) in msg
    _run(eng)  # the refused calls left the dense-scope cells in place
    dense_rows = eng.cost_cells()
    want = c.rows(o)
    _eq(dense_rows, want[dm[want[:, 0].astype(np.int64)]])
    eng.set_page_cost(None, scope=ALL)
    for getter in (eng.cost_cells, lambda: eng.report_page_cost("/nonexistent"),
                   lambda: eng.object_blocks(2, source=COST)):
        assert code(getter)[0] == STATE
    assert _lib.lib.nmg_count_cost_cells(eng.h) == STATE
    _run(eng)  # (the kernels run without the cells again)
    eng.set_page_cost(**kw, scope=ALL)
    eng.set_objects(rp.table)  # drops the cells, the sparse ones too
    assert code(eng.cost_cells)[0] == STATE
    eng.close()
    from numamma_amd.engine import Engine
    multi = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=T, devices=[0, 0])
    multi.set_objects(rp.table)
    assert code(lambda: multi.set_page_cost(**kw, scope=ALL))[0] == INVALID
    multi.close()


# ---- 9. the dense scope is nmg_set_page_cost

@pytest.mark.parametrize("o", cx.OPTION_SETS, ids=cx.OPTION_IDS)
def test_scope_dense_is_set_page_cost(huge, o):
    c = huge
    want = c.dump.dense_rows(o)
    plain = _run(_engine(c.rp, o, scope=DENSE))  # (Engine.set_page_cost calls nmg_set_page_cost)
    _eq(plain.cost_cells(), want)
    plain.close()
    eng = _engine(c.rp, o, scope=DENSE)
    opt = _lib.nmg_page_cost_options(o.bucket_mask, o.access_mask, o.metric, 0, 0)
    assert _lib.lib.nmg_set_page_cost_ex(eng.h, C.byref(opt), DENSE) == 0
    _run(eng)
    _eq(eng.cost_cells(), want)
    assert not np.isin(want[:, 0], [c.role["H"], c.role["M"], c.st]).any()
    eng.close()
