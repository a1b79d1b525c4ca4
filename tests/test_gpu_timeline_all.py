"""The access timeline of every entry (nmg_set_timeline_ex, NMG_TL_SCOPE_ALL):
the sparse entries -- [stack], objects past the per-entry cap, whatever the
histogram budget left sparse -- keep their non-zero cells in the timeline
sparse table, (ordinal, bin, thread, row) -> u32 count.

Every expectation comes from the oracle, on the CPU, before an engine runs
(timeline_all_expect.py): the lines of its -D dump for the non-stack entries,
sparse or not, binned in numpy; for [stack], which the dump omits and which
matches only ts = 0 samples, its page cells in bin 0.  Each case asserts exact
row equality and the invariant against eng.page_cells(): the rows summed over
the bins are the page cells of every selected entry grouped by row.  The rows
must be equal on attribute_kernel (the small table with a truly huge object)
and on every variant of the partition-first path, under every histogram
budget.  All engines use sparse_capacity = CAP but the table-full case."""
import ctypes as C
import os

import numpy as np
import pytest

import cost_expect as cx
import timeline_all_expect as ax
import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd.replay import MEM_DYNAMIC, SynthConfig, generate, online_alarms, table_at
from test_gpu_page_cost_all import Case as CostCase
from test_gpu_page_cost_all import _large_with_stack
from test_gpu_placement_huge import ALL_SPARSE, CAP, DEFAULT_BUDGET, _kinds, _mid_budget, dense_model
from test_gpu_timeline import DUMPS, TINY_POOL, VARIANT_IDS, VARIANTS, _ent_objs, _samples, escape_replay

pytestmark = pytest.mark.gpu

STATE, INVALID, CAPACITY = -6, -1, -8
ALL, DENSE = _lib.NMG_TL_SCOPE_ALL, _lib.NMG_TL_SCOPE_DENSE
OPTS = tx.TlOpts()
ONE_BIN = tx.TlOpts(nb_bins=1)
HOT_VARIANTS = [0, TINY_POOL, _lib.NMG_F_SINGLE_PASS]
HOT_IDS = ["route", "tinypool", "single"]
BUDGETS = ["default", "mid", "one-cell"]


class Case:
    """A replay, the oracle's results and dump directory, and the expected rows
    per option set -- each checked, when made, to cover the oracle's page cells."""

    def __init__(self, rp, d, role=None):
        self.rp, self.role = rp, role
        self.raw, self.odir = tx.run_oracle(rp, d)
        self.st = ax.stack_entry(rp.table)
        self._rows = {}

    def rows(self, o=OPTS):
        if o not in self._rows:
            r = ax.expected_rows_all(self.odir, self.raw, self.rp.table, o)
            ax.check_covers(r, self.raw, self.rp.table, o)
            r.setflags(write=False)
            self._rows[o] = r
        return self._rows[o]

    def dense_rows(self, o=OPTS):
        """The dense scope's rows under the default budget (timeline_expect's own)."""
        return tx.expected_rows(self.odir, self.rp.table, self.rp.nb_threads, o)[0]

    def budget(self, name):
        return {"default": 0, "mid": _mid_budget(self.rp.table), "one-cell": ALL_SPARSE}[name]

    def dense(self, budget):
        return dense_model(self.rp.table, self.rp.nb_threads, budget or DEFAULT_BUDGET)


def _engine(rp, flags=_lib.NMG_F_DEFAULT, o=OPTS, budget=0, scope=ALL, resident=False, cap=CAP, submit=True, **kw):
    """An engine over rp's table with the timeline set and rp's buffers submitted."""
    import torch
    from numamma_amd.engine import Engine

    eng = Engine(flags=flags, nb_threads=rp.nb_threads, hist_budget_bytes=budget, sparse_capacity=cap)
    eng.set_objects(rp.table)
    eng.set_timeline(**o.kw(), scope=scope, **kw)
    if not submit:
        return eng
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


def _check_invariant(eng, rp, rows, o=OPTS):
    sel = ax.selected_all(rp.table, o)
    assert np.array_equal(tx.sum_over_bins(rows), tx.page_cells_by_row(eng.page_cells(), sel, o.row_shift))


def _check(eng, case, o=OPTS, times=1):
    rows = eng.timeline_cells()
    want = case.rows(o).copy()
    want[:, 4] *= times
    assert rows.dtype == np.uint32 and rows.shape == want.shape and np.array_equal(rows, want)
    _check_invariant(eng, case.rp, rows, o)
    return rows


def _code(fn):
    with pytest.raises(_lib.NmgError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def _routed(eng, extra):
    assert (eng.route_count() == 0) if extra & _lib.NMG_F_SINGLE_PASS else (eng.route_count() > 0)


# ---- the cases

@pytest.fixture(scope="module")
def huge(tmp_path_factory):
    rp, role = ax.huge_replay_tl(OPTS)
    c = Case(rp, str(tmp_path_factory.mktemp("tla_huge")), role)
    H, M, st = role["H"], role["M"], role["stack"]
    r = c.rows()
    ids = r[:, 0]
    assert c.st == st and all((ids == e).any() for e in (H, M, st))
    assert (ids < M).sum() > 20 and ((ids > M) & (ids < H)).sum() > 20  # dense entries on both sides of M
    hb = set(r[ids == H][:, 1].tolist())
    assert len(hb) >= 4 and {0, OPTS.nb_bins - 1} <= hb
    assert (r[ids == st][:, 1] == 0).all() and (r[ids == st][:, 3] == ax.hx.STACK_PAGE).any()
    dm = c.dense(0)
    assert not dm[[H, M, st]].any() and dm.sum() == dm.shape[0] - 3
    assert rp.table.keys.shape[0] <= 1023  # attribute_kernel
    return c


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    """LARGE_CFG with 24 records aimed at two pages of [stack]: 721 entries plus [stack] selected."""
    c = Case(_large_with_stack(), str(tmp_path_factory.mktemp("tla_large")))
    table = c.rp.table
    assert table.keys.shape[0] > 1023
    sel = ax.selected_all(table, OPTS)
    assert int(sel.sum()) == 722 and sel[c.st] and int(sel.sum()) <= ax.MAX_SPARSE
    r = c.rows()
    assert set(np.unique(r[:, 1]).tolist()) == set(range(OPTS.nb_bins))
    assert int(r[r[:, 0] == c.st][:, 4].sum()) == 24 and (r[r[:, 0] == c.st][:, 1] == 0).all()
    dm = c.dense(c.budget("mid"))
    assert dm[r[:, 0]].sum() > 300 and (~dm[r[:, 0]]).sum() > 300  # expected rows of both kinds at the mid budget
    assert np.array_equal(r[c.dense(0)[r[:, 0]]], c.dense_rows())  # the default budget: [stack] alone is sparse
    return c


# ---- 1. small table: attribute_kernel, H and M past the per-entry cap, [stack]

@pytest.mark.parametrize("resident", [False, True], ids=["staged", "resident"])
def test_small_table(huge, resident):
    c = huge
    eng = _run(_engine(c.rp, resident=resident))
    assert eng.route_count() == 0
    ns, nd = _kinds(eng, c.raw, c.rp.table, 0)
    assert nd > 1000 and ns == int(np.isin(c.raw.cells[:, 0], [c.role[k] for k in ("H", "M", "stack")]).sum())
    rows = _check(eng, c)
    ids = rows[:, 0].astype(np.int64)
    assert np.all(np.diff(ids) >= 0) and ids[-1] == c.role["stack"]  # the sparse rows between the dense ones, in id order
    eng.close()


def test_small_table_coarse_rows(huge):
    o = tx.TlOpts(row_shift=3, min_object_bytes=65536)
    eng = _run(_engine(huge.rp, o=o))
    rows = _check(eng, huge, o)
    assert (rows[:, 0] == huge.role["H"]).any() and (rows[rows[:, 0] == huge.role["stack"]][:, 3] == ax.hx.STACK_PAGE >> 3).all()
    eng.close()


# ---- 2. large table: every route variant and the single-pass kernel, under every budget

@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("budget", BUDGETS)
def test_large_table_variants(large, budget, extra):
    c = large
    b = c.budget(budget)
    eng = _run(_engine(c.rp, _lib.NMG_F_DEFAULT | extra, budget=b, resident=True))
    _routed(eng, extra)
    ns, nd = _kinds(eng, c.raw, c.rp.table, b)
    assert (nd == 0) if budget == "one-cell" else (nd > 1000)
    assert (ns > 1000) if budget != "default" else (ns < 10)  # the default budget: [stack]'s two pages alone
    _check(eng, c)
    eng.close()


# ---- 3. scope equivalence

@pytest.mark.parametrize("which", ["huge", "large"])
def test_scope_equivalence(huge, large, which):
    c = huge if which == "huge" else large
    want = c.dense_rows()
    for how in ("plain", "ex"):
        eng = _engine(c.rp, scope=DENSE, submit=False)  # (Engine.set_timeline with the dense scope: nmg_set_timeline)
        if how == "ex":
            o = _lib.nmg_timeline_options(OPTS.t0, OPTS.bin_shift, OPTS.nb_bins, OPTS.row_shift, 0, OPTS.min_object_bytes, 0)
            assert _lib.lib.nmg_set_timeline_ex(eng.h, C.byref(o), DENSE) == 0
        eng.submit_replay(c.rp)
        _run(eng)
        rows = eng.timeline_cells()
        assert rows.shape == want.shape and np.array_equal(rows, want), how
        eng.close()
    eng = _run(_engine(c.rp))
    rows = eng.timeline_cells()
    assert np.array_equal(rows[c.dense(0)[rows[:, 0]]], want) and rows.shape[0] > want.shape[0]
    eng.close()


def test_scope_on_the_all_sparse_budget(large):
    c = large
    eng = _run(_engine(c.rp, budget=ALL_SPARSE, scope=DENSE))
    assert eng.timeline_cells().shape == (0, 5)
    eng.set_timeline(**OPTS.kw(), scope=ALL)
    eng.reset()
    _run(eng)
    _check(eng, c)
    eng.close()


# ---- 4. everything at once: levels, sample matches, cost cells of every entry and the timeline of every entry

@pytest.fixture(scope="module")
def large_cost(large, tmp_path_factory):
    return CostCase(large.rp, str(tmp_path_factory.mktemp("tla_cost")))


@pytest.mark.parametrize("extra", [0, _lib.NMG_F_SINGLE_PASS], ids=["route", "single"])
def test_everything_at_once(large, large_cost, extra):
    c = large
    co = cx.MEMORY_WEIGHT
    eng = _engine(c.rp, DUMPS | extra, budget=c.budget("mid"), submit=False)
    eng.set_page_cost(**co.kw(), scope=_lib.NMG_COST_SCOPE_ALL)
    eng.submit_replay(c.rp)
    _run(eng)
    _routed(eng, extra)
    _check(eng, c)
    ent = c.raw.entries  # (the oracle's levels as object_levels() lays them out)
    assert np.array_equal(eng.object_levels(), np.stack([ent[:, 3:40], ent[:, 42:79]], axis=1))
    large_cost.check(eng.cost_cells(), co)
    eng.close()


# ---- 5. escaped compact records

@pytest.fixture(scope="module")
def escape(tmp_path_factory):
    c = Case(escape_replay(), str(tmp_path_factory.mktemp("tla_esc")))
    r = c.rows()
    dm = c.dense(c.budget("mid"))
    assert r.shape[0] > 10_000 and (~dm[r[:, 0]]).sum() > 300 and dm[r[:, 0]].sum() > 300
    lines = tx._columns(os.path.join(c.odir, "all_memory_accesses.dat"), 4)
    # matched samples from before the table's tbase (their timestamp is the re-read absolute one): bin 0.  Their
    # entries have low ids, dense at the mid budget, so the one-cell budget runs too: there they are sparse
    assert int((lines[:, 1] < np.uint64(OPTS.t0 - (1 << 31))).sum()) > 0
    return c


@pytest.mark.parametrize("extra", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("budget", ["mid", "one-cell"])
def test_escaped_records(escape, budget, extra):
    c = escape
    eng = _run(_engine(c.rp, _lib.NMG_F_DEFAULT | extra, budget=c.budget(budget), resident=True))
    _routed(eng, extra)
    _check(eng, c)
    eng.close()


# ---- 6. one hot sparse cell

def _hot(rp, e, skip, page=2, th=6):
    """About 30 % of rp's records -- whole buffers past the first `skip`, given
    to thread th -- rewritten to one page of entry e, their timestamps inside bin 5."""
    ent = rp.table.entries
    lo, hi = OPTS.t0 + (5 << OPTS.bin_shift), OPTS.t0 + (6 << OPTS.bin_shift)
    assert int(ent["alloc_date"][e]) <= lo and int(ent["free_date"][e]) >= hi and int(ent["buffer_size"][e]) >= (page + 1) * tx.PAGE
    rng = np.random.default_rng(7)
    total = sum(r.shape[0] for r in _samples(rp))
    n = 0
    for b, rec in list(zip(rp.buffers, _samples(rp)))[skip:]:
        if n >= 0.3 * total:
            break
        k = rec.shape[0]
        b.thread_rank = th
        rec["addr"] = ent["buffer_addr"][e] + np.uint64(page * tx.PAGE) + rng.integers(0, tx.PAGE, k, dtype=np.uint64)
        rec["timestamp"] = rng.integers(lo, hi, k, dtype=np.uint64)
        n += k
    assert 0.28 < n / total < 0.4
    return n


def _assert_hot(c, e, n, page=2, th=6):
    r = c.rows()
    top = r[np.argmax(r[:, 4])]
    assert tuple(top[:4]) == (e, 5, th, page) and n * 0.9 <= top[4] <= n and top[4] >= 4096


@pytest.fixture(scope="module")
def hot_huge(tmp_path_factory):
    rp, role = ax.huge_replay_tl(OPTS)
    n = _hot(rp, role["H"], 4)  # (the first four buffers carry the plan's records)
    c = Case(rp, str(tmp_path_factory.mktemp("tla_hot_h")), role)
    _assert_hot(c, role["H"], n)
    return c


@pytest.fixture(scope="module")
def hot_large(tmp_path_factory):
    rp = _large_with_stack()
    ent = rp.table.entries
    lo, hi = OPTS.t0 + (5 << OPTS.bin_shift), OPTS.t0 + (6 << OPTS.bin_shift)
    ok = (ent["mem_type"] == MEM_DYNAMIC) & (ent["alloc_date"] <= lo) & (ent["free_date"] >= hi) & \
         (ent["buffer_size"] >= 3 * tx.PAGE)
    e = int(np.argmax(np.where(ok, ent["buffer_size"], 0)))
    assert ok[e]
    n = _hot(rp, e, 1)  # (the first buffer carries the stack's records)
    c = Case(rp, str(tmp_path_factory.mktemp("tla_hot_l")))
    _assert_hot(c, e, n)
    return c


@pytest.mark.parametrize("extra", HOT_VARIANTS, ids=HOT_IDS)
@pytest.mark.parametrize("which", ["huge", "large"])
def test_hot_sparse_cell(hot_huge, hot_large, which, extra):
    """Thousands of records on one key: whole waves insert and add the same key
    from many workgroups -- the case a CAS race would break."""
    c, budget = (hot_huge, 0) if which == "huge" else (hot_large, ALL_SPARSE)
    eng = _run(_engine(c.rp, _lib.NMG_F_DEFAULT | extra, budget=budget, resident=True))
    if which == "large":
        _routed(eng, extra)
    _check(eng, c)
    eng.close()


# ---- 7. accumulate and reset

def test_accumulate_and_reset(large):
    c = large
    eng = _engine(c.rp, budget=c.budget("mid"), resident=True)
    eng.analyze()
    eng.analyze()
    eng.synchronize()
    _run(eng)
    _check(eng, c, times=3)
    eng.reset()
    assert eng.timeline_cells().shape == (0, 5)
    _run(eng)
    _check(eng, c)
    for scope in (DENSE, ALL):
        eng.set_timeline(**OPTS.kw(), scope=ALL)
        eng.set_timeline(None, scope=scope)
        for getter in (eng.timeline_cells, lambda: eng.report_timeline("/nonexistent")):
            assert _code(getter)[0] == STATE
    _run(eng)  # (and the kernels run without it again)
    eng.close()


def test_reset_with_nothing_inserted(large):
    c = large
    eng = _engine(c.rp, budget=c.budget("mid"))
    eng.reset()
    eng.reset()
    assert eng.timeline_cells().shape == (0, 5)
    _run(eng)
    _check(eng, c)
    eng.close()


# ---- 8. streamed chunks and a recorded online run

def test_streamed_chunks(large):
    from numamma_amd.engine import Engine

    c = large
    rp = c.rp
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=c.budget("mid"), sparse_capacity=CAP)
    eng.set_objects(rp.table)
    eng.set_timeline(**OPTS.kw(), scope=ALL)
    eng.stream_begin(chunk_bytes=2 << 20)
    for r, a, data in rp.linear_buffers():
        eng.submit_buffer(data, r, a)
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    assert eng.route_count() >= 2
    _check(eng, c)
    eng.close()


def test_recorded_online_run():
    """nmg_set_objects with the final table, the timeline of every entry, then
    alarm tables listing subsets of its ids.  The oracle writes no dumps in
    alarm mode: the invariant against page_cells() is the check."""
    from numamma_amd.engine import Engine, table_objects

    rp = generate(SynthConfig(nb_samples=120_000, nb_intervals=2_000, nb_threads=4, with_stack=False, reuse_frac=0.2,
                              buffer_records=500, seed=72))
    rp.buffers.reverse()  # online: oldest ring first
    t = rp.table
    snaps = [(be,) + table_at(t, ts) for be, ts in online_alarms(rp, 5)]
    dm0 = dense_model(t, rp.nb_threads, DEFAULT_BUDGET)
    npg = t.entries["buffer_size"].astype(np.int64) // tx.PAGE + 1
    mid = int(npg[dm0].sum()) * rp.nb_threads * 4 // 2
    dm = dense_model(t, rp.nb_threads, mid)
    sel = ax.selected_all(t, OPTS)
    assert 100 < int((sel & ~dm).sum()) <= ax.MAX_SPARSE and int((sel & dm).sum()) > 100
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=mid, sparse_capacity=CAP)
    eng.set_objects(t)
    eng.set_timeline(**OPTS.kw(), scope=ALL)
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
    assert eng.route_count() > 0
    rows = eng.timeline_cells()
    assert (dm[rows[:, 0]]).sum() > 300 and (~dm[rows[:, 0]]).sum() > 300
    assert np.all(np.diff(rows[:, 0].astype(np.int64)) >= 0)
    _check_invariant(eng, rp, rows)
    eng.update_objects(t.keys, t.entry_off, np.arange(t.nb_entries, dtype=np.uint32), table_objects(t))
    eng.close()


# ---- 9. errors

def test_errors_and_budget(large):
    from numamma_amd.engine import Engine

    c = large
    rp, table = c.rp, c.rp.table
    kw = OPTS.kw()
    mid = c.budget("mid")
    dm = c.dense(mid)
    sel = ax.selected_all(table, OPTS)
    npg = table.entries["buffer_size"].astype(np.int64) // tx.PAGE + 1
    dense_bytes = int(npg[dm & sel].sum()) * OPTS.nb_bins * rp.nb_threads * 4
    need = dense_bytes + ax.SLOT_BYTES * CAP
    eng = _engine(rp, budget=mid, budget_bytes=need, submit=False)  # the budget itself
    assert _code(lambda: eng.set_timeline(**kw, scope=2))[0] == INVALID
    assert _code(lambda: eng.set_timeline(**kw, scope=1 << 31))[0] == INVALID
    assert _code(lambda: eng.set_timeline(**kw, scope=ALL, reserved=1))[0] == INVALID
    rc, msg = _code(lambda: eng.set_timeline(**kw, scope=ALL, budget_bytes=need - 1))
    assert rc == CAPACITY and str(need) in msg
    eng.set_timeline(**kw, scope=DENSE, budget_bytes=dense_bytes)  # the dense scope needs the dense cells only
    rc, msg = _code(lambda: eng.set_timeline(**kw, scope=DENSE, budget_bytes=dense_bytes - 1))
    assert rc == CAPACITY and str(dense_bytes) in msg
    eng.close()
    # more than 1023 selected sparse entries
    every = tx.TlOpts(min_object_bytes=0)
    nsel = int(ax.selected_all(table, every).sum())
    assert nsel == table.nb_entries > ax.MAX_SPARSE
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=ALL_SPARSE, sparse_capacity=CAP)
    eng.set_objects(table)
    rc, msg = _code(lambda: eng.set_timeline(**every.kw(), scope=ALL))
    assert rc == CAPACITY and str(nsel) in msg and "min_object_bytes" in msg and "hist_budget_bytes" in msg
    assert _code(eng.timeline_cells)[0] == STATE  # nothing was set
    eng.set_timeline(**every.kw(), scope=DENSE)  # no entry is dense: nothing selected, nothing refused
    eng.close()
    multi = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, devices=[0, 0], sparse_capacity=CAP)
    multi.set_objects(table)
    assert _code(lambda: multi.set_timeline(**kw, scope=ALL))[0] == INVALID
    multi.close()


def _full_replay():
    """150 pages of H, eight records each by one thread, the eight in eight bins."""
    plan = [("H", 10 * p, ax.hx.T_N3, 8) for p in range(150)]  # (the thread whose buffer holds 1200 records)
    rp, role = ax.hx.huge_replay(plan=plan)
    ent = rp.table.entries
    H = role["H"]
    lo, size = int(ent["buffer_addr"][H]), int(ent["buffer_size"][H])
    stamps = np.array([OPTS.t0 + (k << OPTS.bin_shift) + 3 for k in range(8)], dtype=np.uint64)
    assert int(ent["alloc_date"][H]) <= int(stamps[0]) and int(stamps[-1]) <= int(ent["free_date"][H])
    for rec in _samples(rp):
        hit = np.flatnonzero((rec["addr"] >= np.uint64(lo)) & (rec["addr"] < np.uint64(lo + size)))
        rec["timestamp"][hit] = stamps[np.arange(hit.shape[0]) % 8]
    return rp, role


def test_table_full(tmp_path):
    rp, role = _full_replay()
    c = Case(rp, str(tmp_path / "o"), role)
    dm = c.dense(0)
    cells = c.raw.cells
    npage = int((~dm[cells[:, 0]]).sum())  # the sparse page table's keys
    ntl = int((~dm[c.rows()[:, 0]]).sum())  # the timeline sparse table's keys
    assert npage <= 512 and ntl > 1024 and int((~dm[c.rows(ONE_BIN)[:, 0]]).sum()) <= 512
    eng = _engine(rp, cap=1 << 10)
    rc, msg = _code(lambda: _run(eng))
    assert rc == CAPACITY
    eng.reset()
    eng.set_timeline(**ONE_BIN.kw(), scope=ALL)
    _run(eng)
    _check(eng, c, ONE_BIN)
    eng.close()


# ---- 10. the per-site files

def test_report_timeline(tmp_path, huge):
    c = huge
    o = tx.TlOpts(min_object_bytes=0)  # every entry
    want = tx.expected_site_files(c.odir, o)
    assert len(want) > 20
    eng = _run(_engine(c.rp, o=o))
    rows = _check(eng, c, o)
    d = str(tmp_path / "out")
    eng.report(d, str(tmp_path / "e.txt"))
    before = tx.read_dir(d, "")
    eng.report_timeline(d)
    eng.close()
    after = tx.read_dir(d, "")
    got = tx.read_dir(d, "callsite_timeline_")
    assert got == want  # the oracle's per-site dumps, binned; the same ids; none for the stack site
    assert {n: s for n, s in after.items() if not n.startswith("callsite_timeline_")} == before
    # H's and M's own sites: a file each whose lines are the object's rows
    for e in (c.role["H"], c.role["M"]):
        r = rows[rows[:, 0] == e]
        text = "#thread_rank timestamp offset count\n" + "".join(
            f"{th} {o.t0 + (b << o.bin_shift)} {rw << 12} {n}\n" for _, b, th, rw, n in r.tolist())
        assert sum(1 for s in got.values() if s == text) == 1
    assert not any(f" {ax.hx.STACK_PAGE << 12} " in s for s in got.values())
