"""The page cost cells and the access timeline merged across engines by hand:
the dense arrays as NMG_ARR_COST64 / NMG_ARR_TL32 through nmg_cells_pack and
nmg_cells_unpack_add, the sparse parts through nmg_sparse_export_ex, a sum by
key on the host and nmg_sparse_import_ex -- the steps distributed.merge_engine
chains (test_gpu_distributed_cells.py runs that chain over two ranks).

Every expectation comes from the oracle, on the CPU, before an engine runs:
cost rows from cost_expect / cost_all_expect (the -D dump's lines, [stack]
through Case.check), timeline rows from timeline_expect / timeline_all_expect,
blocks from placement_expect.  The two inputs are the smallest that reach
every path: the small table with H and M past the per-entry cap and [stack]
(attribute_kernel), and LARGE_CFG (the partition-first path) at the mid and
the all-sparse histogram budget.  All engines run on device 0."""
import os

import numpy as np
import pytest

import cost_all_expect as ax
import cost_expect as cx
import placement_expect as px
import placement_huge_expect as hx
import timeline_all_expect as tax
import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd.distributed import merge_sparse_u64, shard_ranges
from numamma_amd.replay import SynthConfig, generate
from test_gpu_page_cost_all import LARGE_CFG
from test_gpu_page_cost_all import Case as CostCase
from test_gpu_placement_huge import ALL_SPARSE, CAP, _mid_budget, dense_model

pytestmark = pytest.mark.gpu

INVALID, STATE, RANGE, CAPACITY = -1, -6, -7, -8
COST64, TL32 = _lib.NMG_ARR_COST64, _lib.NMG_ARR_TL32
COUNTS, COST, TIMELINE = _lib.NMG_SPARSE_PAGE_COUNTS, _lib.NMG_SPARSE_PAGE_COST, _lib.NMG_SPARSE_TIMELINE
ALL, DENSE = 1, 0
assert (_lib.NMG_COST_SCOPE_ALL, _lib.NMG_TL_SCOPE_ALL) == (ALL, ALL)
OPTS = tx.TlOpts()
EVERY_ENTRY = tx.TlOpts(min_object_bytes=0)  # what the oracle's per-site dumps cover
DEFAULT_BUDGET = 4 << 30


def _dev():
    import torch

    return torch.device("cuda", 0)


def _code(fn):
    with pytest.raises(_lib.NmgError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def _engine(rp, budget=0, cost=None, cost_scope=ALL, tl=None, tl_scope=ALL, shard=None):
    """An engine over rp's table with the products set and rp's buffers (shard =
    (rank, world): that rank's byte-balanced range, device resident, with its
    seq_base) analysed."""
    import torch
    from numamma_amd.engine import Engine

    eng = Engine(nb_threads=rp.nb_threads, hist_budget_bytes=budget, sparse_capacity=CAP)
    eng.set_objects(rp.table)
    if cost is not None:
        eng.set_page_cost(**cost.kw(), scope=cost_scope)
    if tl is not None:
        eng.set_timeline(**tl.kw(), scope=tl_scope)
    if shard is None:
        eng.submit_replay(rp)
    else:
        arena, offs, lens, ranks, acc = rp.packed()
        lo, hi = shard_ranges(lens, shard[1])[shard[0]]
        assert hi > lo
        base, end = int(offs[lo]), int(offs[hi - 1] + lens[hi - 1])
        eng._arena = torch.from_numpy(arena[base:end].copy()).to(_dev())  # (lives as long as the engine)
        eng.set_device_buffers(eng._arena.data_ptr(), offs[lo:hi] - base, lens[lo:hi], ranks[lo:hi], acc[lo:hi],
                               seq_base=lo)
    eng.analyze()
    eng.synchronize()
    return eng


def _export(eng, which):
    """The merge array `which` as a numpy array (u64, or u32 for the timeline)."""
    import torch

    n = eng.array_size(which)
    t = torch.empty(max(n, 1), dtype=torch.int32 if which in (TL32, _lib.NMG_ARR_HIST32) else torch.int64, device=_dev())
    eng.export_array(which, t.data_ptr())
    a = t[:n].cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint64)


def _pack(eng, which, cap=None):
    """(n, the list tensor of max(cap, 1) pairs); cap None: exactly the list's length."""
    import torch

    if cap is None:
        cap = eng.cells_pack(which, 0, 0)  # (no list: the length alone)
    lst = torch.empty(2 * max(cap, 1), dtype=torch.int64, device=_dev())
    torch.cuda.synchronize(_dev())
    return eng.cells_pack(which, lst.data_ptr(), cap), lst


def _pairs(lst, n):
    return lst[:2 * n].cpu().numpy().view(np.uint64).reshape(-1, 2)


def _device_pairs(pairs):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.uint64).view(np.int64).reshape(-1)).to(_dev())
    torch.cuda.synchronize(_dev())
    return t


def _merge_products(a, b):
    """b's cost and timeline cells into a: the dense lists added, the sparse kinds summed by key and imported
    (the page counts first: their import zeroes the sparse cost cells)."""
    parts = {k: [a.sparse_export_ex(k), b.sparse_export_ex(k)] for k in (COUNTS, COST, TIMELINE)}
    for which in (COST64, TL32):
        assert a.array_size(which) == b.array_size(which)
        n, lst = _pack(b, which)
        a.cells_unpack_add(which, lst.data_ptr(), n)
    for k in (COUNTS, COST, TIMELINE):
        a.sparse_import_ex(k, *merge_sparse_u64(parts[k]))
    return {k: [p[0].shape[0] for p in parts[k]] for k in parts}


def _merge_counters(a, b):
    """b's counters into a, as merge_engine's dense reduces do: what the reports' site ids are made from."""
    import torch

    flip = -(1 << 63)
    for which, op in ((_lib.NMG_ARR_SUM64, "sum"), (_lib.NMG_ARR_MIN64, "min"), (_lib.NMG_ARR_MAX64, "max"),
                      (_lib.NMG_ARR_HIST32, "sum")):
        n = a.array_size(which)
        assert n == b.array_size(which)
        if not n:
            continue
        dt = torch.int32 if which == _lib.NMG_ARR_HIST32 else torch.int64
        ta, tb = torch.empty(n, dtype=dt, device=_dev()), torch.empty(n, dtype=dt, device=_dev())
        a.export_array(which, ta.data_ptr())
        b.export_array(which, tb.data_ptr())
        if op == "sum":
            ta += tb
        else:  # (unsigned order on int64 bits)
            f = torch.minimum if op == "min" else torch.maximum
            ta = f(ta ^ flip, tb ^ flip) ^ flip
        torch.cuda.synchronize(_dev())
        a.import_array(which, ta.data_ptr())
    (sa, fa), (sb, fb) = a.buffer_counts(), b.buffer_counts()
    a.set_buffer_counts(np.concatenate([sa, sb]), np.concatenate([fa, fb]),
                        np.asarray(list(a.buffer_bytes) + list(b.buffer_bytes), dtype=np.uint64))


def _tl_eq(rows, want, times=1):
    w = want.copy()
    w[:, 4] *= times
    assert rows.dtype == np.uint32 and rows.shape == w.shape and np.array_equal(rows, w)


# ---- the inputs and the oracle's expectations

def _tl_rows(c, o):
    r = tax.expected_rows_all(c.odir, c.raw, c.rp.table, o)
    tax.check_covers(r, c.raw, c.rp.table, o)
    r.setflags(write=False)
    return r


@pytest.fixture(scope="module")
def huge(tmp_path_factory):
    rp, role = hx.huge_replay(stack=True)
    c = CostCase(rp, str(tmp_path_factory.mktemp("merge_huge")), role)
    assert rp.table.keys.shape[0] <= 1023  # attribute_kernel
    ok = cx.dense(rp.table, rp.nb_threads)
    H, M = role["H"], role["M"]
    assert c.st == role["stack"] and not ok[H] and not ok[M]
    want = c.rows(cx.EVERYTHING)[:, 0]
    assert (want == H).any() and (want == M).any() and ok[want.astype(np.int64)].sum() > 20
    c.tl = {o: _tl_rows(c, o) for o in (OPTS, EVERY_ENTRY)}
    ids = c.tl[OPTS][:, 0]
    assert all((ids == e).any() for e in (H, M, c.st)) and ok[ids].sum() > 20  # sparse and dense timeline rows
    c.budgets = {"default": 0}
    return c


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    c = CostCase(generate(LARGE_CFG), str(tmp_path_factory.mktemp("merge_large")))
    table, T = c.rp.table, c.rp.nb_threads
    assert table.keys.shape[0] > 1023  # the partition-first path
    c.mid = _mid_budget(table)
    dm = dense_model(table, T, c.mid)
    r = c.rows(cx.MEMORY_WEIGHT)[:, 0].astype(np.int64)
    assert dm[r].sum() > 300 and (~dm[r]).sum() > 300  # expected cost rows of both kinds at the mid budget
    c.tl = {OPTS: _tl_rows(c, OPTS)}
    t = c.tl[OPTS][:, 0]
    assert dm[t].sum() > 300 and (~dm[t]).sum() > 300  # and timeline rows of both kinds
    assert int(tax.selected_all(table, OPTS).sum()) <= tax.MAX_SPARSE
    c.budgets = {"mid": c.mid, "one-cell": ALL_SPARSE}
    return c


INPUTS = [("huge", "default"), ("large", "mid"), ("large", "one-cell")]
INPUT_IDS = ["huge", "large-mid", "large-one-cell"]


def _input(huge, large, which):
    c = huge if which[0] == "huge" else large
    return c, c.budgets[which[1]]


# ---- 1. pack round trip

def _tl_size(table, T, o):
    size = table.entries["buffer_size"].astype(np.uint64)
    sel = tx.selected(table, T, o)
    return int(o.nb_bins) * T * int((size[sel] // np.uint64(4096) + np.uint64(1)).sum())


@pytest.mark.parametrize("threads", [3, 7, 8])
def test_pack_round_trip(threads):
    import torch
    from numamma_amd.engine import Engine

    rp = generate(SynthConfig(nb_samples=30_000, nb_intervals=300, nb_threads=threads, seed=190 + threads))
    # five bins, and the first size threshold that leaves a timeline of 4k + 1, 2 or 3 cells (T odd): the partial last quad
    tl = next(o for o in (tx.TlOpts(nb_bins=5, min_object_bytes=4096 * k) for k in range(1, 64))
              if _tl_size(rp.table, threads, o) % 4 or threads % 2 == 0)
    eng = _engine(rp, cost=cx.EVERYTHING, cost_scope=DENSE, tl=tl, tl_scope=DENSE)
    sizes = {COST64: eng.array_size(_lib.NMG_ARR_HIST32), TL32: _tl_size(rp.table, threads, tl)}
    assert threads == 8 or sizes[TL32] % 4
    for which in (COST64, TL32):
        assert eng.array_size(which) == sizes[which] > 0
        ref = _export(eng, which)
        nz = np.flatnonzero(ref)
        assert nz.shape[0] > 100
        n, lst = _pack(eng, which, cap=sizes[which])
        assert n == nz.shape[0] == eng.cells_pack(which, 0, 0)
        p = _pairs(lst, n)
        assert np.array_equal(p[:, 0], nz.astype(np.uint64))  # ascending, unique, the non-zero cells
        assert np.array_equal(p[:, 1], ref[nz].astype(np.uint64))
        # a short list: the full length, and nothing past cap pairs written
        cap = n // 2
        guard = torch.full((2 * n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=_dev())
        torch.cuda.synchronize(_dev())
        assert eng.cells_pack(which, guard.data_ptr(), cap) == n
        g = guard.cpu().numpy().view(np.uint64)
        assert np.array_equal(g[:2 * cap].reshape(-1, 2), p[:cap]) and (g[2 * cap:] == 0x5A5A5A5A5A5A5A5A).all()
        # the list alone gives the array back
        eng.reset()
        assert not _export(eng, which).any() and eng.cells_pack(which, 0, 0) == 0
        eng.cells_unpack_add(which, lst.data_ptr(), n)
        assert np.array_equal(_export(eng, which), ref)
        eng.reset()  # (the next array's cells as the analysis leaves them)
        eng.analyze()
        eng.synchronize()
    eng.close()
    plain = Engine(nb_threads=rp.nb_threads)  # neither product: both arrays empty
    plain.set_objects(rp.table)
    for which in (COST64, TL32):
        assert plain.array_size(which) == 0 and plain.cells_pack(which, 0, 0) == 0
        plain.cells_unpack_add(which, 0, 0)
    plain.close()


# ---- 2. nmg_cells_unpack_add

@pytest.mark.parametrize("which", [COST64, TL32], ids=["cost64", "tl32"])
def test_unpack_add(which):
    rp = generate(SynthConfig(nb_samples=2_000, nb_intervals=100, nb_threads=4, seed=197))
    eng = _engine(rp, cost=cx.EVERYTHING, cost_scope=DENSE, tl=tx.TlOpts(nb_bins=3), tl_scope=DENSE)
    eng.reset()
    n = eng.array_size(which)
    assert n > 1000
    big = (1 << 40) + 3 if which == COST64 else (1 << 31) + 3
    pairs = [(5, 7), (n - 1, 1), (5, 11), (n + 10, 0), (6, 0), (5, big), (n - 1, 2), (n // 2, 9), (1 << 40, 0)]
    lst = _device_pairs(pairs)
    eng.cells_unpack_add(which, lst.data_ptr(), len(pairs))
    want = np.zeros(n, dtype=np.uint64)
    want[5], want[n - 1], want[n // 2] = 18 + big, 3, 9
    assert np.array_equal(_export(eng, which).astype(np.uint64), want)
    eng.cells_unpack_add(which, lst.data_ptr(), len(pairs))  # adds, never overwrites
    assert np.array_equal(_export(eng, which).astype(np.uint64), (2 * want) & (~np.uint64(0) if which == COST64 else np.uint64(0xFFFFFFFF)))
    bad = _device_pairs([(3, 1), (n, 1)])
    rc, msg = _code(lambda: eng.cells_unpack_add(which, bad.data_ptr(), 2))
    assert rc == RANGE and "nmg_cells_unpack_add" in msg
    for other in (_lib.NMG_ARR_HIST32, _lib.NMG_ARR_SUM64, 6, -1):
        assert _code(lambda: eng.cells_unpack_add(other, lst.data_ptr(), 1))[0] == INVALID
        assert _code(lambda: eng.cells_pack(other, lst.data_ptr(), 1))[0] == INVALID
    assert _code(lambda: eng.cells_unpack_add(which, 0, 1))[0] == INVALID  # a null list
    assert _code(lambda: eng.cells_pack(which, 0, 1))[0] == INVALID
    eng.cells_unpack_add(which, 0, 0)
    eng.close()
    from numamma_amd.engine import Engine
    fresh = Engine(nb_threads=4)  # before a table exists
    assert _code(lambda: fresh.cells_pack(which, 0, 0))[0] == INVALID
    assert _code(lambda: fresh.cells_unpack_add(which, 0, 0))[0] == INVALID
    fresh.close()


# ---- 3. doubling: both engines analyse the whole replay, every cell overlaps

@pytest.mark.parametrize("o", [cx.MEMORY_WEIGHT, cx.EVERYTHING], ids=["weight", "count"])
@pytest.mark.parametrize("which", INPUTS, ids=INPUT_IDS)
def test_doubling(huge, large, which, o):
    c, budget = _input(huge, large, which)
    a = _engine(c.rp, budget, cost=o, tl=OPTS)
    b = _engine(c.rp, budget, cost=o, tl=OPTS)
    once = a.cost_cells()
    c.check(once, o)
    n = _merge_products(a, b)
    dm = dense_model(c.rp.table, c.rp.nb_threads, budget or DEFAULT_BUDGET)
    assert n[COUNTS][0] > 0 and n[TIMELINE][0] > 0 and n[COST] == [int((~dm[once[:, 0].astype(np.int64)]).sum())] * 2
    rows = a.cost_cells()
    c.check(rows, o, times=2)
    assert np.array_equal(rows, ax.with_times(once, 2))
    _tl_eq(a.timeline_cells(), c.tl[OPTS], times=2)
    a.close()
    b.close()


# ---- 4. sharded: the byte-balanced halves, merged by hand, equal the oracle's unsharded run

def _sharded(c, budget, o, tl, cost_scope=ALL, tl_scope=ALL):
    a = _engine(c.rp, budget, cost=o, cost_scope=cost_scope, tl=tl, tl_scope=tl_scope, shard=(0, 2))
    b = _engine(c.rp, budget, cost=o, cost_scope=cost_scope, tl=tl, tl_scope=tl_scope, shard=(1, 2))
    assert a.global_counters()[1] > 0 and b.global_counters()[1] > 0
    _merge_counters(a, b)
    n = _merge_products(a, b)
    b.close()
    assert np.array_equal(a.page_cells(), c.raw.cells)
    return a, n


@pytest.mark.parametrize("o", cx.OPTION_SETS, ids=cx.OPTION_IDS)
@pytest.mark.parametrize("budget", ["mid", "one-cell"])
def test_sharded_large(tmp_path, large, budget, o):
    c = large
    table, T = c.rp.table, c.rp.nb_threads
    a, _ = _sharded(c, c.budgets[budget], o, OPTS)
    c.check(a.cost_cells(), o)
    _tl_eq(a.timeline_cells(), c.tl[OPTS])
    if budget == "mid":  # the per-site files and blocks.dat, sites with a dense and a sparse member
        mats = cx.site_matrices(c.odir, T, o)
        want = cx.site_files(mats)
        assert len(want) > (50 if o != cx.REMOTE_READS else 0)
        d = str(tmp_path / "cost")
        a.report_page_cost(d)
        assert cx.read_dir(d, "") == want
        po = px.Opts(4, density_threshold=0)
        d2 = str(tmp_path / "place")
        a.report_placement(d2, **po.kw(), source=_lib.NMG_PLACE_PAGE_COST)
        text = cx.site_blocks_text(c.odir, table, mats, po)
        assert text.count("begin_block") > 0 and open(os.path.join(d2, "blocks.dat")).read() == text
    a.close()


@pytest.mark.parametrize("o", cx.OPTION_SETS, ids=cx.OPTION_IDS)
def test_sharded_huge(tmp_path, huge, o):
    c = huge
    table, T = c.rp.table, c.rp.nb_threads
    a, n = _sharded(c, 0, o, EVERY_ENTRY)
    rows = a.cost_cells()
    c.check(rows, o)
    _tl_eq(a.timeline_cells(), c.tl[EVERY_ENTRY])
    # the blocks of the non-stack entries from the dump's rows, H and M (sparse cost cells) among them
    po = px.Opts(4, (0, 0, 1, 1, 3, 3, 3, 3), 0)
    got = a.object_blocks(**po.kw(), source=_lib.NMG_PLACE_PAGE_COST)
    want = ax.object_blocks_all(c.rows(o), table, T, po)
    assert got.dtype == np.uint64 and np.array_equal(got[got[:, 0] != c.st], want)
    if o == cx.EVERYTHING:
        assert (want[:, 0] == c.role["H"]).any() and (want[:, 0] == c.role["M"]).any()
    # callsite_timeline_<id>.dat: the oracle's per-site dumps, binned
    wantf = tx.expected_site_files(c.odir, EVERY_ENTRY)
    assert len(wantf) > 20
    d = str(tmp_path / "tl")
    a.report_timeline(d)
    assert tx.read_dir(d, "callsite_timeline_") == wantf
    a.close()


def test_sharded_dense_scope(large):
    """Scope DENSE on both products: the sparse kinds export no pair, the rows are the dense entries' rows."""
    c, o = large, cx.MEMORY_WEIGHT
    dm = dense_model(c.rp.table, c.rp.nb_threads, c.mid)
    a, n = _sharded(c, c.mid, o, OPTS, cost_scope=DENSE, tl_scope=DENSE)
    assert n[COST] == [0, 0] and n[TIMELINE] == [0, 0] and min(n[COUNTS]) > 0
    want = c.rows(o)
    got = a.cost_cells()
    assert got.dtype == np.uint64 and np.array_equal(got, want[dm[want[:, 0].astype(np.int64)]])
    t = c.tl[OPTS]
    _tl_eq(a.timeline_cells(), t[dm[t[:, 0]]])
    a.close()


# ---- 5. the sparse kinds: errors, the page counts through _ex, reset

def test_sparse_import_errors(large):
    from numamma_amd.engine import Engine

    c, o = large, cx.MEMORY_WEIGHT
    rp = c.rp
    dm = dense_model(rp.table, rp.nb_threads, c.mid)
    u64 = np.uint64
    eng = _engine(rp, c.mid, cost=o, tl=OPTS)
    k0, v0 = eng.sparse_export()
    e0 = eng.sparse_export_ex(COUNTS)
    assert e0[1].dtype == np.uint64 and np.array_equal(e0[0], k0) and np.array_equal(e0[1], v0.astype(u64))
    kc, vc = eng.sparse_export_ex(COST)
    kt, vt = eng.sparse_export_ex(TIMELINE)
    for k, v in ((k0, e0[1]), (kc, vc), (kt, vt)):
        assert k.shape[0] > 300 and np.all(k[1:] > k[:-1]) and v.all()
    assert np.isin(kc, k0).all()  # a cost implies a count
    assert np.array_equal(kt, tax.sparse_keys(c.tl[OPTS], rp.table, dm, OPTS))
    rows = eng.cost_cells()
    assert (~dm[rows[:, 0].astype(np.int64)]).sum() == kc.shape[0]
    # the same pairs back: the same rows
    eng.sparse_import_ex(COST, kc, vc)
    eng.sparse_import_ex(TIMELINE, kt, vt)
    assert np.array_equal(eng.cost_cells(), rows)
    _tl_eq(eng.timeline_cells(), c.tl[OPTS])
    # a cost key absent from the page table
    absent = next(u64(k) for k in (k0[-1] + u64(1), k0[-1] + u64(2), k0[0] - u64(1)) if k not in set(k0.tolist()))
    rc, msg = _code(lambda: eng.sparse_import_ex(COST, np.append(kc, absent), np.append(vc, u64(5))))
    assert rc == INVALID and "1 cost keys absent" in msg
    left = eng.cost_cells()
    assert np.array_equal(left, rows[dm[rows[:, 0].astype(np.int64)]])  # no sparse row left, the dense ones untouched
    assert eng.sparse_export_ex(COST)[0].shape[0] == 0
    # values of 2^32 or more: the u32 kinds refuse them, the cost keeps them
    for kind, k, v in ((COUNTS, k0, e0[1]), (TIMELINE, kt, vt)):
        w = v.copy()
        w[3] = u64(1) << u64(32)
        assert _code(lambda: eng.sparse_import_ex(kind, k, w))[0] == RANGE
    eng.sparse_import_ex(COUNTS, k0, e0[1])
    w = vc.copy()
    w[3] = (u64(1) << u64(40)) + u64(1)
    eng.sparse_import_ex(COST, kc, w)
    assert np.array_equal(eng.sparse_export_ex(COST)[1], w)
    # the timeline table's capacity
    many = np.arange(CAP + 1, dtype=u64)
    assert _code(lambda: eng.sparse_import_ex(TIMELINE, many, np.ones(CAP + 1, dtype=u64)))[0] == CAPACITY
    # any other kind
    for fn in (lambda: eng.sparse_import_ex(3, kc, vc), lambda: eng.sparse_export_ex(3)):
        assert _code(fn)[0] == INVALID
    assert _lib.lib.nmg_sparse_count_ex(eng.h, 3) == INVALID
    # after an import, a reset leaves every kind empty
    eng.sparse_import_ex(TIMELINE, kt, vt)
    eng.reset()
    for kind in (COUNTS, COST, TIMELINE):
        assert eng.sparse_export_ex(kind)[0].shape[0] == 0
    assert eng.cost_cells().shape == (0, 4) and eng.timeline_cells().shape == (0, 5)
    eng.close()
    # engines without the sparse parts
    dense = Engine(nb_threads=rp.nb_threads, hist_budget_bytes=c.mid, sparse_capacity=CAP)
    dense.set_objects(rp.table)
    one = (kc[:1], vc[:1])
    assert _code(lambda: dense.sparse_import_ex(COST, *one))[0] == STATE  # no cost cells at all
    assert _code(lambda: dense.sparse_import_ex(TIMELINE, kt[:1], vt[:1]))[0] == STATE  # no timeline
    dense.set_page_cost(**o.kw(), scope=DENSE)
    dense.set_timeline(**OPTS.kw(), scope=DENSE)
    assert _code(lambda: dense.sparse_import_ex(COST, *one))[0] == STATE  # the dense scope
    assert _code(lambda: dense.sparse_import_ex(TIMELINE, kt[:1], vt[:1]))[0] == STATE
    for kind in (COST, TIMELINE):  # nothing to import is no error
        dense.sparse_import_ex(kind, kc[:0], vc[:0])
        assert dense.sparse_export_ex(kind)[0].shape[0] == 0
    dense.close()
