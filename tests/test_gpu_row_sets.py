"""The contract the four device-side row products share (DESIGN.md "Row sets"):
page cells, timeline cells, cost cells and object blocks are prepared once per
results epoch by their nmg_count_* call, stay on the device, and are copied
out by nmg_get_*, which refuses another row count.

Tiny inputs (7 entries, one key with two entries, 2 threads, two buffers of 64
SAMPLE records, attribute_kernel): what is pinned here is the cache, not the
attribution.  Every expected row comes from the oracle: its page cells
(pyoracle's raw results), and timeline_expect / cost_expect / placement_expect
over its dump files."""
import ctypes as C
import os

import numpy as np
import pytest

import cost_expect as cx
import placement_expect as px
import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd._lib import lib
from numamma_amd.replay import ObjectTable, SynthConfig, generate
from test_gpu_placement_huge import dense_model

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -6
FLAGS = _lib.NMG_F_DEFAULT | _lib.NMG_F_SINGLE_PASS
T = 2
CFG = SynthConfig(nb_samples=128, nb_intervals=5, nb_threads=T, size_min=4096, size_max=40_000, reuse_frac=0.3,
                  realloc_frac=0.0, nb_globals=1, with_stack=False, site_ratio=0.6, read_frac=1.0, buffer_records=64,
                  frac_stack=0.0, seed=38)

TL, TL2 = tx.TlOpts(), tx.TlOpts(bin_shift=31, nb_bins=3, row_shift=1, min_object_bytes=0)
COST, COST2 = cx.MEMORY_WEIGHT, cx.EVERYTHING
PO = px.Opts(2, None, 0)  # (threshold 0: doubling the counts keeps the blocks' pages)
PO_OTHERS = [px.Opts(1, None, 0), px.Opts(2, (1, 0), 0), px.Opts(2, None, 2)]  # another N, map, threshold
PRODUCTS = ["cells", "timeline", "cost", "blocks"]


class Tiny:
    """The replay, the oracle's results over it, and the expected rows of every product."""

    def __init__(self, rp, d):
        self.rp = rp
        self.raw, self.odir = cx.run_oracle(rp, d)
        self.dump = cx.Dump(self.odir, rp.table, rp.nb_threads)

    def expect(self, p, opt=None, times=1):
        t = self.rp.table
        if p == "cells":
            rows, col = self.raw.cells.astype(np.uint32).copy(), 3
        elif p == "timeline":
            rows, col = tx.expected_rows(self.odir, t, T, opt or TL)[0], 4
        elif p == "cost":
            rows, col = self.dump.rows(opt or COST)[0], 3
        else:
            po, source = opt or (PO, 0)
            if source == _lib.NMG_PLACE_PAGE_COST:  # (the engine's cost cells are COST's)
                assert times == 1
                return cx.object_blocks(self.dump.rows(COST)[0], t, T, po)
            return px.object_rows(self.raw, t, po, times)  # (no sparse entry: NMG_PLACE_HUGE changes nothing)
        rows[:, col] *= rows.dtype.type(times)
        return rows


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    rp = generate(CFG)
    t = rp.table
    assert t.nb_entries == 7 and int((np.diff(t.entry_off.astype(np.int64)) == 2).sum()) == 1  # one reused address
    assert [len(b.ring) // 40 for b in rp.buffers] == [64, 64] and {b.thread_rank for b in rp.buffers} == {0, 1}
    c = Tiny(rp, str(tmp_path_factory.mktemp("row_sets")))
    assert dense_model(t, T, 4 << 30).all()
    for p in PRODUCTS:  # every product has rows, and the second option sets give other rows
        assert c.expect(p).shape[0] > 4, p
    assert not np.array_equal(c.expect("timeline", TL2), c.expect("timeline"))
    assert c.expect("cost", COST2).shape[0] > c.expect("cost").shape[0]
    return c


# ---- the raw calls

WIDTH = {"cells": (4, np.uint32), "timeline": (5, np.uint32), "cost": (4, np.uint64), "blocks": (5, np.uint64)}
VALUE_COL = {"cells": 3, "timeline": 4, "cost": 3, "blocks": 4}


def _po(opt):
    po, source = opt or (PO, 0)
    return _lib.placement_options(T, source=source, **po.kw())


def count(eng, p, opt=None):
    if p == "cells":
        return lib.nmg_count_page_cells(eng.h)
    if p == "timeline":
        return lib.nmg_count_timeline_cells(eng.h)
    if p == "cost":
        return lib.nmg_count_cost_cells(eng.h)
    po, keep = _po(opt)
    n = lib.nmg_count_object_blocks(eng.h, C.byref(po))
    del keep
    return n


def get(eng, p, n, opt=None, null=False):
    """(return code, the rows array handed in): n rows asked for; null: a NULL pointer."""
    w, dt = WIDTH[p]
    rows = np.full((n + 1, w), 0xA5, dtype=dt)  # (one row more than asked for: a refused call writes nothing)
    ct = C.c_uint32 if dt == np.uint32 else C.c_uint64
    ptr = None if null else rows.ctypes.data_as(C.POINTER(ct))
    if p == "blocks":
        po, keep = _po(opt)
        rc = lib.nmg_get_object_blocks(eng.h, C.byref(po), ptr, n)
        del keep
    else:
        rc = {"cells": lib.nmg_get_page_cells, "timeline": lib.nmg_get_timeline_cells,
              "cost": lib.nmg_get_cost_cells}[p](eng.h, ptr, n)
    assert (rows[n] == 0xA5).all()  # never past n rows
    return rc, rows[:n]


def last_error(eng):
    buf = C.create_string_buffer(512)
    lib.nmg_get_last_error_detail(eng.h, buf, 512)
    return buf.value.decode(errors="replace")


def fetch(eng, p, opt=None):
    """count, then get: the rows (asserting both calls succeed)."""
    n = count(eng, p, opt)
    assert n >= 0, (p, n, last_error(eng))
    rc, rows = get(eng, p, n, opt)
    assert rc == OK, (p, rc, last_error(eng))
    return rows


def same(rows, want):
    return rows.dtype == want.dtype and rows.shape == want.shape and rows.tobytes() == want.tobytes()


def engine(rp, table=None, products=PRODUCTS, **kw):
    """An engine over the table with the products' cells set and rp's buffers submitted."""
    from numamma_amd.engine import Engine

    eng = Engine(flags=FLAGS, nb_threads=T, **kw)
    eng.set_objects(table or rp.table)
    if "timeline" in products:
        eng.set_timeline(**TL.kw())
    if "cost" in products:
        eng.set_page_cost(**COST.kw())
    eng.submit_replay(rp)
    return eng


def run(eng):
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() == 0  # attribute_kernel
    return eng


# ---- 1. one epoch: the rows are prepared once and read any number of times

@pytest.mark.parametrize("p", PRODUCTS)
def test_same_epoch(tiny, p):
    eng = run(engine(tiny.rp))
    want = tiny.expect(p)
    n1, n2 = count(eng, p), count(eng, p)
    assert n1 == n2 == want.shape[0]
    (rc1, a), (rc2, b) = get(eng, p, n1), get(eng, p, n2)
    assert (rc1, rc2) == (OK, OK)
    assert same(a, b) and same(a, want), p
    eng.close()


# ---- 2. another row count is refused; no rows: n == 0 and no pointer needed

@pytest.mark.parametrize("p", PRODUCTS)
def test_wrong_n(tiny, p):
    eng = run(engine(tiny.rp))
    n = count(eng, p)
    assert n == tiny.expect(p).shape[0] > 1
    for bad, null in ((n - 1, False), (n + 1, False), (0, True), (0, False)):
        rc, _ = get(eng, p, bad, null=null)
        assert rc == INVALID and "row count mismatch" in last_error(eng), (p, bad)
    rc, rows = get(eng, p, n)  # (and the refused calls left the rows alone)
    assert rc == OK and same(rows, tiny.expect(p))
    if n:
        assert get(eng, p, n, null=True)[0] == INVALID  # rows without a pointer
    eng.close()


@pytest.mark.parametrize("p", PRODUCTS)
def test_no_rows(tiny, p):
    """The same buffers over the table moved 2^40 up: nothing matches."""
    rp = tiny.rp
    t = rp.table
    ent = t.entries.copy()
    ent["buffer_addr"] += np.uint64(1 << 40)
    far = ObjectTable(t.keys + np.uint64(1 << 40), t.entry_off, ent, t.callstack_pool, t.string_pool)
    eng = run(engine(rp, table=far))
    assert eng.global_counters()[1:] == (128, 0)  # every sample read, none matched
    assert count(eng, p) == 0
    assert get(eng, p, 0, null=True)[0] == OK
    rc, _ = get(eng, p, 1)
    assert rc == INVALID and "row count mismatch" in last_error(eng)
    eng.close()


# ---- 3. what ends an epoch

@pytest.mark.parametrize("p", PRODUCTS)
def test_invalidation(tiny, p):
    eng = run(engine(tiny.rp))
    once = fetch(eng, p)
    assert same(once, tiny.expect(p))
    run(eng)  # the same buffers again, no reset
    twice = fetch(eng, p)
    col = VALUE_COL[p]
    keys = [c for c in range(once.shape[1]) if c != col]
    assert same(twice, tiny.expect(p, times=2))
    assert np.array_equal(twice[:, keys], once[:, keys]) and np.array_equal(twice[:, col], 2 * once[:, col])
    eng.reset()
    assert count(eng, p) == 0 and get(eng, p, 0, null=True)[0] == OK
    run(eng)
    assert same(fetch(eng, p), tiny.expect(p))
    if p in ("timeline", "cost"):  # other options: fresh cells, and the rows are theirs
        other = TL2 if p == "timeline" else COST2
        (eng.set_timeline if p == "timeline" else eng.set_page_cost)(**other.kw())
        assert count(eng, p) == 0
        run(eng)
        assert same(fetch(eng, p), tiny.expect(p, other))
    eng.close()


# ---- 4. the object blocks' rows belong to their options as well

def test_blocks_keyed_by_options(tiny):
    eng = run(engine(tiny.rp))
    opts = [(PO, 0)] + [(o, 0) for o in PO_OTHERS] + [(PO, _lib.NMG_PLACE_PAGE_COST), (PO, _lib.NMG_PLACE_HUGE)]
    wants = [tiny.expect("blocks", o) for o in opts]
    assert len({w.tobytes() for w in wants[:5]}) == 5  # every option matters (HUGE: no sparse entry, PO's rows)
    assert same(wants[5], wants[0])
    for a in range(len(opts)):
        for b in range(len(opts)):  # count with a, then count and get with b, in one epoch
            assert count(eng, "blocks", opts[a]) == wants[a].shape[0]
            assert count(eng, "blocks", opts[b]) == wants[b].shape[0]
            rc, rows = get(eng, "blocks", wants[b].shape[0], opts[b])
            assert rc == OK and same(rows, wants[b]), (a, b)
    # a get after a count with other options: prepared for its own options, not served the counted rows
    a, b = opts[0], opts[3]
    na, nb = wants[0].shape[0], wants[3].shape[0]
    assert na != nb
    assert count(eng, "blocks", a) == na
    rc, rows = get(eng, "blocks", nb, b)
    assert rc == OK and same(rows, wants[3])
    assert count(eng, "blocks", a) == na
    rc, _ = get(eng, "blocks", na, b)
    assert rc == INVALID and "row count mismatch" in last_error(eng)
    eng.close()


# ---- 5. page cells and cost cells share the per-entry work arrays

@pytest.mark.parametrize("order", [("cells", "cost"), ("cost", "cells")], ids=["cells-first", "cost-first"])
def test_interleaving(tiny, order):
    eng = run(engine(tiny.rp))
    first, second = order
    n1, n2 = count(eng, first), count(eng, second)
    (rc1, r1), (rc2, r2) = get(eng, first, n1), get(eng, second, n2)
    assert (rc1, rc2) == (OK, OK)
    assert same(r1, tiny.expect(first)) and same(r2, tiny.expect(second))
    # and with a new epoch between the two counts' gets
    run(eng)
    n1 = count(eng, first)
    n2 = count(eng, second)
    rc2, r2 = get(eng, second, n2)
    rc1, r1 = get(eng, first, n1)
    assert (rc1, rc2) == (OK, OK)
    assert same(r1, tiny.expect(first, times=2)) and same(r2, tiny.expect(second, times=2))
    eng.close()


# ---- 6. page cells whose entry lies in the sparse table

def _one_sparse_budget(tiny):
    """(budget, entry): the entry with most cells among those a budget can make the only sparse one."""
    t = tiny.rp.table
    npg = t.entries["buffer_size"].astype(np.int64) // 4096 + 1
    ncell = np.bincount(tiny.raw.cells[:, 0], minlength=t.nb_entries)
    for e in np.argsort(-ncell).tolist():
        budget = int(npg.sum() - npg[e]) * T * 4
        if (~dense_model(t, T, budget)).tolist() == [i == e for i in range(t.nb_entries)]:
            return budget, e
    raise AssertionError("no budget leaves exactly one entry sparse")


@pytest.mark.parametrize("kind", ["one-sparse", "no-dense"])
def test_page_cells_with_sparse_entries(tiny, kind):
    want = tiny.expect("cells")
    if kind == "one-sparse":
        budget, e = _one_sparse_budget(tiny)
        assert int((want[:, 0] == e).sum()) > 1  # the entry has rows
    else:
        budget = 4  # one cell: no entry gets dense cells
    eng = run(engine(tiny.rp, products=(), hist_budget_bytes=budget, sparse_capacity=1 << 10))
    nsparse = lib.nmg_sparse_count(eng.h)
    if kind == "one-sparse":
        assert nsparse == int((want[:, 0] == e).sum()) and eng.array_size(_lib.NMG_ARR_HIST32) > 0
    else:
        assert nsparse == want.shape[0] and eng.array_size(_lib.NMG_ARR_HIST32) == 0  # tab.cells() == 0
    n1, n2 = count(eng, "cells"), count(eng, "cells")
    assert n1 == n2 == want.shape[0]
    (rc1, a), (rc2, b) = get(eng, "cells", n1), get(eng, "cells", n2)
    assert (rc1, rc2) == (OK, OK) and same(a, b) and same(a, want)
    rc, _ = get(eng, "cells", n1 - 1)
    assert rc == INVALID and "row count mismatch" in last_error(eng)
    # the results snapshot of the same engine: the same rows
    eng.results_begin()
    snap = np.array(eng.results_end()[7])  # (cells [nb_cells, 4])
    assert snap.shape[0] == want.shape[0] and same(snap, want)
    # the exported sparse cells: keys ascending, and decoded (sparse idx:22 | thread:10 | page:32; sparse idx ->
    # entry in id order) exactly the oracle's rows of the sparse entries
    keys, vals = eng.sparse_export()
    assert keys.dtype == np.uint64 and vals.dtype == np.uint32 and np.all(keys[1:] > keys[:-1])
    sparse_ids = np.flatnonzero(~dense_model(tiny.rp.table, T, budget))
    assert (keys >> np.uint64(42) < sparse_ids.shape[0]).all()
    decoded = np.stack([sparse_ids[(keys >> np.uint64(42)).astype(np.int64)], (keys >> np.uint64(32)) & np.uint64(0x3ff),
                        keys & np.uint64(0xffffffff), vals], axis=1).astype(np.uint32)
    assert same(decoded, want[np.isin(want[:, 0], sparse_ids)])
    eng.close()


def test_snapshot_of_an_empty_table(tiny):
    """E = 0: the snapshot has no cell, and its counts are the synchronous getters'."""
    eng = run(engine(tiny.rp, table=ObjectTable.empty(), products=()))
    g, ns, nf = eng.global_counters()
    bs, bf = eng.buffer_counts()
    assert (ns, nf) == (128, 0) and bs.tolist() == [64, 64]
    assert count(eng, "cells") == 0
    eng.results_begin()
    got = eng.results_end()
    assert got[7].shape == (0, 4)  # nb_cells == 0
    assert np.array_equal(got[0], g) and (got[1], got[2]) == (ns, nf)
    assert np.array_equal(np.array(got[3]), bs) and np.array_equal(np.array(got[4]), bf)
    assert got[5].shape[0] == 0 and got[6].shape[0] == 0  # no entry
    eng.close()


# ---- 7. a live online table: the reports' rows follow the walk order

def _report_all(eng, d):
    os.makedirs(d)
    eng.report(d, os.path.join(d, "stdout.txt"))
    eng.report_timeline(d)
    eng.report_page_cost(d)
    eng.report_placement(d, **PO.kw())
    return tx.read_dir(d, "")


def test_live_online_table(tiny, tmp_path):
    """One nmg_update_objects listing every object under ids that are not the
    table order (test_gpu_online.py's live case, one alarm): the four reports
    are those of the same objects given in id order, and the oracle's."""
    from numamma_amd.engine import Engine, table_objects

    rp = tiny.rp
    t = rp.table
    ids = np.arange(t.nb_entries, dtype=np.uint32)[::-1].copy()  # walk order != id order
    o = tx.TlOpts(min_object_bytes=0)
    outs = []
    for live in (False, True):
        eng = Engine(flags=FLAGS, nb_threads=T)
        if live:
            eng.set_objects(ObjectTable.empty())
            eng.update_objects(t.keys, t.entry_off, ids, table_objects(t))
            eng.table = t  # the reports' metadata, in the table's order
        else:
            eng.set_objects(t)
        eng.set_timeline(**o.kw())
        eng.set_page_cost(**COST.kw())
        eng.submit_replay(rp)
        run(eng)
        if live:  # the getters' rows carry the ids
            cells = fetch(eng, "cells").copy()
            pos = np.empty_like(ids)
            pos[ids] = np.arange(ids.shape[0], dtype=np.uint32)
            cells[:, 0] = pos[cells[:, 0]]
            assert same(cells[np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))], tiny.expect("cells"))
        outs.append(_report_all(eng, str(tmp_path / ("live" if live else "ids"))))
        eng.close()
    by_id, by_walk = outs
    assert sorted(by_walk) == sorted(by_id)
    for name in by_id:
        assert by_walk[name] == by_id[name], name
    # and against the oracle: its report files, and the expectations over its dumps
    _, plain = px.run_oracle(rp, str(tmp_path / "plain"))
    for name in os.listdir(plain):
        assert by_walk[name] == open(os.path.join(plain, name)).read(), name
    want = dict(tx.expected_site_files(tiny.odir, o))
    want.update(cx.site_files(cx.site_matrices(tiny.odir, T, COST)))
    want["blocks.dat"] = px.expected_file(tiny.odir, t, PO)
    assert len(want) > 6 and want["blocks.dat"].count("begin_block") > 1
    extra = {n: s for n, s in by_walk.items() if n not in os.listdir(plain) and n != "stdout.txt"}
    assert extra == want
