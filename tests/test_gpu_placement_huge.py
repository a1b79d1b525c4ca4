"""NMG_PLACE_HUGE on the device: nmg_get_object_blocks and nmg_report_placement
over entries with sparse page cells -- [stack], objects past the dense cap, and
every entry that the histogram budget left without dense cells.

Every expectation comes from the oracle's files: placement_huge_expect.py for
the object rows (the rule over every entry's cells of the raw dump),
placement_expect.expected_file for blocks.dat (the oracle's per-site counter
files sum all of a site's members, sparse or not).  Each engine run asserts
which kinds of cells it had: the sparse table's export against the cells the
oracle has for the entries that CellCursor::place (restated in dense_model)
leaves sparse, and the remaining page cells as dense ones."""
import os

import numpy as np
import pytest

import placement_expect as px
import placement_huge_expect as hx
from numamma_amd import _lib
from numamma_amd.replay import SynthConfig, generate, online_alarms, table_at
from numamma_amd.results import object_blocks_host, report_placement_host
from test_gpu_placement import PRIMARY, Case, _downloaded, _ent_objs, crafted_replay

pytestmark = pytest.mark.gpu

PAGE = px.PAGE
T = 8
HUGE = _lib.NMG_PLACE_HUGE
ALL_SPARSE = 4  # hist_budget_bytes: one cell -- no entry gets dense cells
DEFAULT_BUDGET = 4 << 30
CAP = 1 << 18  # sparse_capacity


def dense_model(table, nb_threads, budget):
    """CellCursor::place over the table in id order: which entries get dense cells."""
    npg = (table.entries["buffer_size"].astype(np.uint64) // np.uint64(PAGE)).astype(object) + 1
    out = np.zeros(table.nb_entries, dtype=bool)
    cells = 0
    for e in range(table.nb_entries):
        n = int(npg[e])
        if n * nb_threads <= (1 << 24) and (cells + n) * nb_threads <= budget // 4 and cells + n < 0xFFFFFFFF:
            out[e] = True
            cells += n
    return out


def _read(d, name="blocks.dat"):
    return open(os.path.join(d, name)).read()


def _engine(rp, budget=0, **kw):
    from numamma_amd.engine import Engine

    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=budget, sparse_capacity=CAP, **kw)
    eng.set_objects(rp.table)
    eng.submit_replay(rp)
    return eng


def _run(rp, budget=0, **kw):
    eng = _engine(rp, budget, **kw)
    eng.analyze()
    eng.synchronize()
    return eng


def _kinds(eng, raw, table, budget, times=1):
    """Assert the engine's cells are of the kinds the budget intends; (sparse, dense) cell counts."""
    dense = dense_model(table, raw.nb_threads, budget or DEFAULT_BUDGET)
    want_sparse = int((~dense[raw.cells[:, 0]]).sum())
    keys, vals = eng.sparse_export()
    assert keys.shape[0] == want_sparse and want_sparse > 0
    n = eng.page_cells().shape[0]
    assert n == raw.cells.shape[0]
    assert int(vals.sum()) == times * int(raw.cells[~dense[raw.cells[:, 0]], 3].sum())
    return want_sparse, n - want_sparse


def _check(eng, case, o, tmp, times=1, online=False):
    want = hx.object_rows_all(case.raw, case.rp.table, o, times)
    got = eng.object_blocks(**o.kw(), source=HUGE)
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), o
    d = str(tmp)
    eng.report_placement(d, online=online, **o.kw(), source=HUGE)
    text = px.expected_file(case.odir, case.rp.table, o, times)
    assert text.count("begin_block") > 10 and _read(d) == text, o
    return want


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("plg_craft"))
    rp, role = crafted_replay(d)
    c = Case(rp, os.path.join(d, "crafted"))
    c.role = role
    return c


@pytest.fixture(scope="module")
def huge(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("plg_huge"))
    rp, role = hx.huge_replay(stack=True)
    c = Case(rp, os.path.join(d, "huge"))
    c.role = role
    c.want = hx.check_huge_expectation(c.raw, rp.table, role, stack=True)  # before any engine runs
    return c


# ---- 1. budget invariance

def _mid_budget(table):
    """Half of what the entries' dense cells take: both kinds occur."""
    dense = dense_model(table, T, DEFAULT_BUDGET)
    npg = table.entries["buffer_size"].astype(np.int64) // PAGE + 1
    return int(npg[dense].sum()) * T * 4 // 2


def test_budget_invariance(tmp_path, crafted):
    c = crafted
    table = c.rp.table
    ent = table.entries
    mid = _mid_budget(table)
    want = hx.object_rows_all(c.raw, table, PRIMARY)
    plain = px.object_rows(c.raw, table, PRIMARY)
    assert hx.blocks(want, c.role["stack"]) == [(0, 5, 5, 20)]
    assert np.array_equal(want[want[:, 0] != c.role["stack"]], plain)
    # the mid budget: a site with a dense and a sparse member; A, B, C (the 63/64/65-page situations) sparse
    dm = dense_model(table, T, mid)
    site = {}
    for e in range(table.nb_entries):
        site.setdefault((table.caller(e), int(ent["initial_buffer_size"][e])), set()).add(bool(dm[e]))
    assert any(len(v) == 2 for v in site.values())
    for i, budget in enumerate((ALL_SPARSE, mid, 0)):
        eng = _run(c.rp, budget)
        ns, nd = _kinds(eng, c.raw, table, budget)
        assert (nd == 0) if budget == ALL_SPARSE else (nd > 0)
        assert (ns > 1000 and nd > 1000) if budget == mid else True
        assert np.array_equal(_check(eng, c, PRIMARY, tmp_path / f"b{i}"), want)
        if budget == 0:  # without the flag: today's rows and file
            assert np.array_equal(eng.object_blocks(**PRIMARY.kw()), plain)
            eng.report_placement(str(tmp_path / "plain"), **PRIMARY.kw())
            assert _read(str(tmp_path / "plain")) == px.expected_file(c.odir, table, PRIMARY)
        eng.close()


# ---- 2. the truly huge object and [stack]

def test_huge_object_and_stack(tmp_path, huge):
    c = huge
    table = c.rp.table
    H, M, st = (c.role[k] for k in ("H", "M", "stack"))
    eng = _run(c.rp)
    ns, nd = _kinds(eng, c.raw, table, 0)
    assert ns == int(np.isin(c.raw.cells[:, 0], [H, M, st]).sum()) and nd > 1000
    o = hx.PRIMARY
    got = eng.object_blocks(**o.kw(), source=HUGE)
    assert got.shape == c.want.shape and np.array_equal(got, c.want)
    host = object_blocks_host(_downloaded(eng, c.rp), table, **o.kw(), source=HUGE)
    assert np.array_equal(host, got)
    assert hx.blocks(got, st) == [(0, hx.STACK_PAGE, hx.STACK_PAGE, 20)] and hx.STACK_PAGE > 1 << 26  # above 2^24
    # the huge groups' rows between the dense groups' rows, in id order
    ids = got[:, 0].astype(np.int64)
    assert np.all(np.diff(ids) >= 0)
    m0 = int(np.flatnonzero(ids == M)[0])
    assert 20 < m0 and ids[m0 - 1] < M and ids[m0 + 2] > M and ids[-1] == st and ids[-2] == H
    plain = eng.object_blocks(**o.kw())
    assert np.array_equal(plain, got[~np.isin(ids, [H, M, st])])
    # blocks.dat: each of the two objects is its own call site; the host writes the same file
    d = str(tmp_path / "dev")
    eng.report_placement(d, **o.kw(), source=HUGE)
    h = str(tmp_path / "host")
    report_placement_host(_downloaded(eng, c.rp), table, h, **o.kw(), source=HUGE)
    assert _read(d) == _read(h)
    sid = {(cl, s): i for i, cl, s in px.read_sites(c.odir)}
    ent = table.entries
    for e in (H, M):
        assert hx.file_blocks(_read(d), sid[(table.caller(e), int(ent["initial_buffer_size"][e]))]) == hx.blocks(got, e)
    assert "[stack]" not in _read(d)
    eng.close()


# ---- 3. list-index boundaries

def test_list_index_boundaries(tmp_path):
    """The huge kernels step over the list of qualifying pages by waves of 64
    items in workgroups of 256 (place_huge_emit_kernel sums a block's counts
    per wave).  M has 320 consecutive qualifying pages, one cell each, so a
    page's list index is its page - 100: the node changes at list indices 63,
    64, 65 and 256 (a workgroup step), one block runs over the wave steps 128
    and 192, and M's list ends at index 320, a wave step, where H -- the next
    huge group -- begins with the node M ended with."""
    n0, n1, n3 = hx.T_A, hx.T_N1, hx.T_N3
    node_thread = [n0] * 63 + [n1] + [n0] + [n3] * 191 + [n1] * 64
    assert len(node_thread) == 320
    plan = [("M", 100 + i, th, 9) for i, th in enumerate(node_thread)] + [("H", p, n1, 9) for p in range(10)]
    rp, role = hx.huge_replay(plan=plan)
    c = Case(rp, str(tmp_path / "oracle"))
    o = hx.PRIMARY
    want = hx.object_rows_all(c.raw, rp.table, o)
    assert hx.blocks(want, role["M"]) == [(0, 100, 162, 63 * 9), (1, 163, 163, 9), (0, 164, 164, 9), (3, 165, 355, 191 * 9),
                                         (1, 356, 419, 64 * 9)]
    assert hx.blocks(want, role["H"]) == [(1, 0, 9, 90)]
    eng = _run(rp)
    ns, nd = _kinds(eng, c.raw, rp.table, 0)
    assert ns == 330 and nd > 1000
    got = eng.object_blocks(**o.kw(), source=HUGE)
    assert got.shape == want.shape and np.array_equal(got, want)
    eng.close()


# ---- 4. empty and degenerate cases

def test_degenerate_cases(tmp_path):
    from numamma_amd.engine import Engine

    # no sparse entry: the flag changes nothing
    rp = generate(SynthConfig(nb_samples=20_000, nb_intervals=300, nb_threads=4, with_stack=False, seed=101))
    c = Case(rp, str(tmp_path / "oracle"))
    o = px.Opts(2, (0, 1, 1, 0), 8)
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, sparse_capacity=CAP)
    eng.set_objects(rp.table)
    assert eng.object_blocks(**o.kw(), source=HUGE).shape == (0, 5)  # before any analysis
    eng.submit_replay(rp)
    eng.analyze()
    eng.synchronize()
    assert eng.sparse_export()[0].shape[0] == 0 and dense_model(rp.table, 4, DEFAULT_BUDGET).all()
    plain = eng.object_blocks(**o.kw())
    assert plain.shape[0] > 20 and np.array_equal(plain, px.object_rows(c.raw, rp.table, o))
    assert np.array_equal(eng.object_blocks(**o.kw(), source=HUGE), plain)
    # source = 6: refused, and the detail says why
    with pytest.raises(_lib.NmgError) as ei:
        eng.object_blocks(**o.kw(), source=_lib.NMG_PLACE_PAGE_COST | HUGE)
    assert ei.value.code == -1 and "sparse entries have no cost cells" in str(ei.value)
    with pytest.raises(_lib.NmgError) as ei:
        eng.report_placement(str(tmp_path / "never"), **o.kw(), source=_lib.NMG_PLACE_PAGE_COST | HUGE)
    assert ei.value.code == -1 and "sparse entries have no cost cells" in str(ei.value)
    for source in (1, 3, 5, 7, 8, 1 << 32):
        with pytest.raises(_lib.NmgError) as ei:
            eng.object_blocks(**o.kw(), source=source)
        assert ei.value.code == -1, source
    assert not os.path.exists(str(tmp_path / "never"))
    eng.close()
    # every entry sparse, before any analysis and with a threshold no cell passes
    eng = _engine(rp, ALL_SPARSE)
    assert eng.object_blocks(**o.kw(), source=HUGE).shape == (0, 5)
    eng.analyze()
    eng.synchronize()
    _kinds(eng, c.raw, rp.table, ALL_SPARSE)
    # one node: cnt(p) is the page's sum over the threads; top, the largest of any object
    page_key, inv = np.unique(c.raw.cells[:, [0, 2]], axis=0, return_inverse=True)
    top = int(np.bincount(inv.reshape(-1), weights=c.raw.cells[:, 3]).max())
    assert eng.object_blocks(nb_nodes=1, density_threshold=top, source=HUGE).shape == (0, 5)
    assert eng.object_blocks(nb_nodes=1, density_threshold=top - 1, source=HUGE).shape[0] >= 1
    assert eng.object_blocks(**o.kw()).shape == (0, 5)  # without the flag: no dense entry, no row
    eng.close()


# ---- 5. paths, every entry sparse

def test_accumulate_and_reset(tmp_path, crafted):
    c = crafted
    eng = _run(c.rp, ALL_SPARSE)
    eng.analyze()
    eng.synchronize()
    _kinds(eng, c.raw, c.rp.table, ALL_SPARSE, times=2)
    twice = _check(eng, c, PRIMARY, tmp_path / "twice", times=2)
    assert not np.array_equal(twice, hx.object_rows_all(c.raw, c.rp.table, PRIMARY))
    eng.reset()
    assert eng.object_blocks(**PRIMARY.kw(), source=HUGE).shape == (0, 5)
    eng.analyze()
    eng.synchronize()
    _kinds(eng, c.raw, c.rp.table, ALL_SPARSE)
    _check(eng, c, PRIMARY, tmp_path / "once")
    eng.close()


def test_streamed_chunks(tmp_path, crafted):
    from numamma_amd.engine import Engine

    rp = crafted.rp
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=ALL_SPARSE, sparse_capacity=CAP)
    eng.set_objects(rp.table)
    eng.stream_begin(chunk_bytes=1 << 20)
    for r, a, data in rp.linear_buffers():
        eng.submit_buffer(data, r, a)
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    _kinds(eng, crafted.raw, rp.table, ALL_SPARSE)
    _check(eng, crafted, PRIMARY, tmp_path / "out")
    eng.close()


def test_recorded_online_run(tmp_path):
    from numamma_amd.engine import Engine, table_objects

    rp = generate(SynthConfig(nb_samples=60_000, nb_intervals=1_000, nb_threads=4, with_stack=False, reuse_frac=0.2,
                              buffer_records=500, seed=72))
    rp.buffers.reverse()  # online: oldest ring first
    t = rp.table
    snaps = [(be,) + table_at(t, ts) for be, ts in online_alarms(rp, 5)]
    c = Case(rp, str(tmp_path / "oracle"), alarms=snaps)
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads, hist_budget_bytes=ALL_SPARSE, sparse_capacity=CAP)
    eng.set_objects(t)
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
    eng.update_objects(t.keys, t.entry_off, np.arange(t.nb_entries, dtype=np.uint32), table_objects(t))
    keys, vals = eng.sparse_export()
    assert keys.shape[0] == c.raw.cells.shape[0] > 1000  # every cell a sparse one
    _check(eng, c, px.Opts(2, (0, 1, 1, 0), 2), tmp_path / "out", online=True)
    eng.close()


def test_two_workers_on_one_device(tmp_path, crafted):
    multi = _run(crafted.rp, ALL_SPARSE, devices=[0, 0])
    _check(multi, crafted, PRIMARY, tmp_path / "multi")
    keys, vals = multi.sparse_export()
    assert keys.shape[0] == crafted.raw.cells.shape[0]
    multi.close()


def test_run_replay_writes_blocks(tmp_path, crafted, huge, monkeypatch):
    from numamma_amd.engine import run_replay

    path = str(tmp_path / "crafted.bin")
    crafted.rp.write(path)
    monkeypatch.setenv("NMG_REPLAY_PLACEMENT", "4:8:huge")
    run_replay(path, str(tmp_path / "c"), str(tmp_path / "c.txt"))
    assert _read(str(tmp_path / "c")) == px.expected_file(crafted.odir, crafted.rp.table, px.Opts(4, None, 8))
    # the replay with the huge objects: their sites appear with the third field only
    path = str(tmp_path / "replay.bin")
    huge.rp.write(path)
    d = str(tmp_path / "out")
    monkeypatch.setenv("NMG_REPLAY_PLACEMENT", "4:8")
    run_replay(path, d, str(tmp_path / "e.txt"))
    plain = _read(d)
    monkeypatch.setenv("NMG_REPLAY_PLACEMENT", "4:8:huge")
    run_replay(path, d, str(tmp_path / "e.txt"))
    o = px.Opts(4, None, 8)
    eng = _run(huge.rp)
    h = str(tmp_path / "eng")
    eng.report_placement(h, **o.kw(), source=HUGE)
    eng.close()
    assert _read(d) == _read(h) and _read(d) != plain
    ent = huge.rp.table.entries
    sid = {(cl, s): i for i, cl, s in px.read_sites(huge.odir)}
    want = hx.object_rows_all(huge.raw, huge.rp.table, o)
    for e in (huge.role["H"], huge.role["M"]):
        s = sid[(huge.rp.table.caller(e), int(ent["initial_buffer_size"][e]))]
        assert hx.file_blocks(_read(d), s) == hx.blocks(want, e) and hx.file_blocks(plain, s) is None
    monkeypatch.setenv("NMG_REPLAY_PLACEMENT", "4:8:vast")
    with pytest.raises(_lib.NmgError):
        run_replay(path, d, str(tmp_path / "e.txt"))
