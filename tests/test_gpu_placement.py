"""NUMA placement on the device: nmg_get_object_blocks and nmg_report_placement.

Every expectation comes from the oracle's files through placement_expect.py
(the rule of include/numamma_gpu.h restated in numpy): the page cells of its
raw dump for the object blocks, its call_sites.log and
callsite_counters_<id>.dat for blocks.dat.

The crafted replay is generate(SynthConfig(60k records, 1500 intervals)) with
sizes up to 1 MiB (the default 256 KiB has no object of 65 or 129 pages), three
large objects cut to exactly 63, 64 and 65 pages, one grown by two pages past
its call site's rows, and the first records of three buffers (whose thread
ranks are set) rewritten to aim at chosen pages of chosen objects, whose other
records are aimed at no object.  The `crafted` fixture asserts, on the
expectation alone and before any engine runs, that the rows contain every
situation the block kernel can get wrong at its 64-page step: see its body.
The primary options are 4 nodes with threads 0-1 on node 0, 2-3 on node 1 and
4-7 on node 3 (node 2 has no thread), threshold 8."""
import os

import numpy as np
import pytest

import placement_expect as px
from numamma_amd import _lib
from numamma_amd.replay import (GLOBAL_BASE, HORIZON, MEM_DYNAMIC, MEM_STACK, RECORD_DTYPE, T0, SynthConfig, generate,
                                online_alarms, table_at)
from numamma_amd.results import GLOBAL_SUMS, RawResults, report_placement_host

pytestmark = pytest.mark.gpu

PAGE = px.PAGE
T = 8
D = 8
PRIMARY = px.Opts(4, (0, 0, 1, 1, 3, 3, 3, 3), D)
T_N0, T_N1, T_N3 = 0, 2, 4  # a thread of node 0, 1 and 3 under PRIMARY
CRAFT_CFG = SynthConfig(nb_samples=60_000, nb_intervals=1_500, size_max=1 << 20, seed=131)


def option_sets(nb_threads):
    """N in {1, 2, 4, T}: the NULL map, the interleaved one, and one that leaves node 0 empty."""
    out = []
    for n in sorted({1, 2, 4, nb_threads}):
        out.append(px.Opts(n, None, D))
        out.append(px.Opts(n, tuple(t % n for t in range(nb_threads)), D))
        if n > 1:
            out.append(px.Opts(n, tuple(1 + t % (n - 1) for t in range(nb_threads)), D))
    return out + [px.Opts(4, None, 0)]


class Case:
    def __init__(self, rp, d, **kw):
        self.rp = rp
        self.raw, self.odir = px.run_oracle(rp, d, **kw)


def _pages(ent, e):
    return int(ent["buffer_size"][e]) // PAGE + 1


def crafted_replay(d):
    """(replay, the chosen entries by role)."""
    rp = generate(CRAFT_CFG)
    t = rp.table
    ent = t.entries
    eo = t.entry_off.astype(np.int64)
    key_of = np.repeat(np.arange(t.nb_keys), np.diff(eo))
    single = np.diff(eo)[key_of] == 1
    nxt = np.append(t.keys[1:], np.uint64(1 << 63))[key_of]
    slack = nxt - (ent["buffer_addr"] + ent["buffer_size"])
    clean = (ent["mem_type"] == MEM_DYNAMIC) & single & (ent["buffer_size"] == ent["initial_buffer_size"])
    npg = ent["buffer_size"].astype(np.int64) // PAGE + 1
    used = set()
    orig_addr, orig_size = ent["buffer_addr"].copy(), ent["buffer_size"].copy()

    def pick(cond, n=1):
        got = [int(e) for e in np.flatnonzero(clean & cond) if int(e) not in used][:n]
        assert len(got) == n
        used.update(got)
        return got if n > 1 else got[0]

    role = {"A": pick(npg >= 130), "B": pick(npg >= 70), "C": pick(npg >= 66)}
    for p in (1, 2):
        role[f"p{p}"] = pick(npg == p)
    for i, p in enumerate((63, 64, 65)):  # cut to size: their own call sites (the size is part of a site's key)
        e = pick(npg >= 66)
        ent["buffer_size"][e] = ent["initial_buffer_size"][e] = (p - 1) * PAGE + 8 * (i + 1)
        role[f"p{p}"] = e
    # call sites with several clean members: (caller, size, callstack or not) groups
    gkey = {}
    for e in np.flatnonzero(clean):
        if int(e) not in used:
            gkey.setdefault((int(ent["caller_off"][e]), int(ent["initial_buffer_size"][e])), []).append(int(e))
    groups = sorted((k, v) for k, v in gkey.items() if len(v) >= 3 and k[1] >= 2 * PAGE)
    assert len(groups) >= 2
    role["S"] = groups[0][1][:3]  # pages that qualify only through the sum of three objects
    used.update(role["S"])
    # an object grown past its site's rows: X (room for two more pages), the site created by Y
    xy = [(k, v) for k, v in groups[1:] if any(slack[e] >= 3 * PAGE for e in v)]
    assert xy
    members = xy[0][1]
    role["X"] = next(e for e in members if slack[e] >= 3 * PAGE)
    role["Y"] = next(e for e in members if e != role["X"])
    ent["buffer_size"][role["X"]] += 2 * PAGE
    used.update((role["X"], role["Y"]))
    role["stack"] = int(np.flatnonzero(ent["mem_type"] == MEM_STACK)[0])

    A, B, C, X, Y = (role[k] for k in "ABCXY")
    R = _pages(ent, Y)
    plan = [  # (entry, page, thread, count); the first record of the analysis creates X's site from Y
        (Y, 0, T_N0, 20),
        (X, 0, T_N1, 20), (X, R + 1, T_N0, 20),
        # A: a block from page 63 into 64; a tie on page 100; exactly D and D + 1; its last page
        (A, 62, T_N0, 20), (A, 63, T_N0, 20), (A, 64, T_N0, 20), (A, 65, T_N0, 20),
        (A, 99, T_N3, 20), (A, 100, T_N0, 15), (A, 100, T_N1, 15), (A, 101, T_N1, 20),
        (A, 110, T_N3, D), (A, 112, T_N3, D + 1),
        (A, _pages(ent, A) - 1, T_N1, 20),
        # B: one block over pages that do not qualify, across the boundary (page 64 at exactly D)
        (B, 60, T_N1, 20), (B, 63, T_N1, 3), (B, 64, T_N1, D), (B, 67, T_N1, 20),
        # C: two blocks of different nodes adjacent at the boundary
        (C, 63, T_N0, 20), (C, 64, T_N3, 20),
        (role["stack"], 5, T_N0, 20),
    ]
    for p in (1, 2, 63, 64, 65):
        plan.append((role[f"p{p}"], p - 1, T_N0, 20))
    plan += [(e, 1, T_N1, 4) for e in role["S"]]
    gvar = int(np.flatnonzero(ent["buffer_addr"] == np.uint64(GLOBAL_BASE))[0])
    plan.append((gvar, 1, T_N3, 20))
    # the generator's own records of the chosen objects (of all of S's call site) aimed at no object
    scrub = sorted(used | set(sum((v for k, v in groups[:1]), [])))
    lo = np.array([int(orig_addr[e]) for e in scrub], dtype=np.uint64)
    hi = lo + np.array([int(orig_size[e]) for e in scrub], dtype=np.uint64)
    order = np.argsort(lo)
    lo, hi = lo[order], hi[order]
    for b in rp.buffers:
        rec = b.ring.view(RECORD_DTYPE)
        k = np.searchsorted(lo, rec["addr"], side="right") - 1
        hit = (k >= 0) & (rec["addr"] < hi[np.maximum(k, 0)])
        rec["addr"][hit] = 8
    # the plan's records: per thread, the first records of one buffer (in analysis order), its rank set
    for b, th in zip(rp.buffers, (T_N0, T_N1, T_N3)):
        rec = b.ring.view(RECORD_DTYPE)
        cells = [(e, p, c) for e, p, t_, c in plan if t_ == th]
        n = sum(c for _, _, c in cells)
        assert b.data_tail == 0 and n < rec.shape[0]
        addr = np.concatenate([np.full(c, int(ent["buffer_addr"][e]) + p * PAGE, dtype=np.uint64) for e, p, c in cells])
        ts = np.concatenate([np.full(c, 0 if e == role["stack"] else T0 + HORIZON // 2, dtype=np.uint64)
                             for e, p, c in cells])
        rec["addr"][:n], rec["timestamp"][:n] = addr, ts
        b.thread_rank = th
    role["R"] = R
    return rp, role


def _blocks(rows, e):
    return [tuple(r) for r in rows[rows[:, 0] == e][:, 1:].tolist()]


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pl_craft"))
    rp, role = crafted_replay(d)
    c = Case(rp, os.path.join(d, "crafted"))
    c.role = role
    ent = rp.table.entries
    o = PRIMARY
    rows = px.object_rows(c.raw, rp.table, o)
    mats = px.object_matrices(c.raw, rp.table)
    sites = px.site_blocks(c.odir, rp.table, o)
    A, B, C, X, Y, R = (role[k] for k in ("A", "B", "C", "X", "Y", "R"))
    assert rp.table.keys.shape[0] > 1023
    # objects of 1, 2, 63, 64, 65 and 129+ pages, each with a block on its last page
    for p in (1, 2, 63, 64, 65):
        e = role[f"p{p}"]
        assert _pages(ent, e) == p and _blocks(rows, e) == [(0, p - 1, p - 1, 20)]
    nA = _pages(ent, A)
    assert nA >= 130 and _blocks(rows, A) == [(0, 62, 65, 80), (3, 99, 99, 20), (0, 100, 100, 15), (1, 101, 101, 20),
                                              (3, 112, 112, D + 1), (1, nA - 1, nA - 1, 20)]  # 63 -> 64 in a block; D + 1 in
    domA, cntA = px.page_dom(mats[A], o)
    assert mats[A][100, T_N0] == mats[A][100, T_N1] == 15 and domA[100] == 0  # the tie: the lower node
    assert cntA[110] == D  # exactly D: out (no block holds page 110)
    # a block that spans pages which do not qualify, across 63 -> 64 (page 64 at exactly D)
    assert _blocks(rows, B) == [(1, 60, 67, 40)]
    assert px.page_dom(mats[B], o)[1][[63, 64]].tolist() == [3, D]
    assert _blocks(rows, C) == [(0, 63, 63, 20), (3, 64, 64, 20)]  # two nodes adjacent at the boundary
    assert set(rows[:, 1].tolist()) == {0, 1, 3}  # node 2 has no thread
    # a site whose page qualifies only through the sum of its objects
    S = role["S"]
    for e in S:
        assert px.page_dom(mats[e], o)[1][1] == 4 and _blocks(rows, e) == []
    s_site = [s for s in sites if (s[1], s[3]) == (rp.table.caller(S[0]), int(ent["initial_buffer_size"][S[0]]))]
    assert len(s_site) == 1 and any(b[0] == 1 and b[1] <= 1 <= b[2] for b in s_site[0][4].tolist())
    s_mat = px.site_matrix(c.odir, s_site[0][0])
    s_members = [e for e in mats if (rp.table.caller(e), int(ent["initial_buffer_size"][e])) == (s_site[0][1], s_site[0][3])]
    assert px.page_dom(s_mat, o)[1][1] > D and all(px.page_dom(mats[e], o)[1][1] <= D for e in s_members)
    # an object with more pages than its site's rows: its own block on page R + 1, none there for the site
    assert _pages(ent, X) == R + 2 and (0, R + 1, R + 1, 20) in _blocks(rows, X)
    x_site = [s for s in sites if (s[1], s[3]) == (rp.table.caller(X), int(ent["initial_buffer_size"][X]))]
    assert len(x_site) == 1 and px.site_matrix(c.odir, x_site[0][0]).shape[0] == R
    assert int(x_site[0][4][:, 2].max()) < R
    # a global-symbol site, and [stack]: cells beyond the threshold, sparse, in no row and no site
    assert any(s[2].startswith("global_var_") for s in sites)
    st = role["stack"]
    assert not px.dense(rp.table, T)[st] and int(c.raw.cells[c.raw.cells[:, 0] == st][:, 3].max()) >= 20
    assert st not in rows[:, 0] and all(s[1] != "[stack]" for s in sites)
    assert len(sites) > 100 and rows.shape[0] > 200
    return c


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return Case(generate(SynthConfig(nb_samples=20_000, nb_intervals=300, nb_threads=4, seed=101)),
                str(tmp_path_factory.mktemp("pl_small")))


# ---- running the engine

def _engine(rp, flags=_lib.NMG_F_DEFAULT, **kw):
    from numamma_amd.engine import Engine

    eng = Engine(flags=flags, nb_threads=rp.nb_threads, **kw)
    eng.set_objects(rp.table)
    eng.submit_replay(rp)
    return eng


def _run(rp, **kw):
    eng = _engine(rp, **kw)
    eng.analyze()
    eng.synchronize()
    return eng


def _read(d, name="blocks.dat"):
    return open(os.path.join(d, name)).read()


def _downloaded(eng, rp):
    """The engine's results as the host functions take them."""
    g, ns, nf = eng.global_counters()
    bs, bf = eng.buffer_counts()
    first, cw = eng.object_counters()
    E = rp.table.nb_entries
    entries = np.zeros((E, 1 + 2 * GLOBAL_SUMS), dtype=np.uint64)
    entries[:, 0] = first
    entries[:, 1], entries[:, 2] = cw[:, 0, 0], cw[:, 0, 1]
    entries[:, 1 + GLOBAL_SUMS], entries[:, 2 + GLOBAL_SUMS] = cw[:, 1, 0], cw[:, 1, 1]
    return RawResults(E, bs.shape[0], rp.nb_threads, g, ns, nf, bs, bf, entries, eng.page_cells())


def _check_objects(eng, case, o, times=1):
    want = px.object_rows(case.raw, case.rp.table, o, times)
    got = eng.object_blocks(**o.kw())
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), o
    return want


def _check_sites(eng, case, o, tmp, times=1, online=False):
    d = str(tmp)
    eng.report_placement(d, online=online, **o.kw())
    want = px.expected_file(case.odir, case.rp.table, o, times)
    assert want.count("begin_block") > 10
    assert _read(d) == want, o


# ---- 1. object blocks

def test_object_blocks_route_path(crafted):
    eng = _run(crafted.rp)
    assert eng.route_count() > 0  # more than 1023 keys: the partition-first path
    n = [_check_objects(eng, crafted, o).shape[0] for o in [PRIMARY] + option_sets(T)]
    assert min(n) > 100 and len(set(n)) > 3  # (the options matter)
    # cached per epoch and options: the same rows again, and other options in between
    first = eng.object_blocks(**PRIMARY.kw())
    eng.object_blocks(nb_nodes=1)
    assert np.array_equal(eng.object_blocks(**PRIMARY.kw()), first)
    eng.close()


@pytest.mark.parametrize("which", ["crafted", "small"])
def test_maps_that_sort_alike_back_to_back(request, which):
    """Two maps with the same N and D under which the thread ranks sorted by
    node are the same list (both non-decreasing), one after the other in one
    results epoch: each call returns its own map's rows."""
    case = request.getfixturevalue(which)
    T_ = case.rp.nb_threads
    first = PRIMARY if T_ == 8 else px.Opts(2, (0, 1, 1, 1), D)
    second = px.Opts(first.nb_nodes, None, D)
    assert list(first.thread_node) == sorted(first.thread_node) and first.node_of(T_).tolist() != second.node_of(T_).tolist()
    eng = _run(case.rp)
    for o in (first, second, first, second):
        _check_objects(eng, case, o)
    assert not np.array_equal(px.object_rows(case.raw, case.rp.table, first), px.object_rows(case.raw, case.rp.table, second))
    eng.close()


def test_object_blocks_small_table(small):
    eng = _run(small.rp)
    assert eng.route_count() == 0  # 309 keys: attribute_kernel
    for o in option_sets(small.rp.nb_threads):
        assert _check_objects(eng, small, o).shape[0] > 20
    eng.close()


# ---- 2. blocks.dat

def test_sites_file(tmp_path, crafted):
    c = crafted
    eng = _run(c.rp)
    d = str(tmp_path / "out")
    eng.report(d, str(tmp_path / "e.txt"))
    before = {n: _read(d, n) for n in os.listdir(d)}
    for i, o in enumerate([PRIMARY, px.Opts(2, None, D), px.Opts(8, tuple(range(8)), 0)]):
        eng.report_placement(d, **o.kw())
        assert _read(d) == px.expected_file(c.odir, c.rp.table, o), o
        h = str(tmp_path / f"host{i}")
        report_placement_host(_downloaded(eng, c.rp), c.rp.table, h, **o.kw())
        assert _read(h) == _read(d)
    after = {n: _read(d, n) for n in os.listdir(d) if n != "blocks.dat"}
    assert after == before  # nmg_report's files are as they were
    eng.close()


def test_accumulate_and_reset(tmp_path, crafted):
    c = crafted
    eng = _run(c.rp)
    eng.analyze()
    eng.synchronize()
    twice = _check_objects(eng, c, PRIMARY, times=2)
    assert not np.array_equal(twice[:, :4], px.object_rows(c.raw, c.rp.table, PRIMARY)[:twice.shape[0], :4])
    _check_sites(eng, c, PRIMARY, tmp_path / "twice", times=2)
    assert _read(str(tmp_path / "twice")) != px.expected_file(c.odir, c.rp.table, PRIMARY)  # the blocks changed
    eng.reset()
    assert eng.object_blocks(**PRIMARY.kw()).shape == (0, 5)
    eng.analyze()
    eng.synchronize()
    _check_objects(eng, c, PRIMARY)
    _check_sites(eng, c, PRIMARY, tmp_path / "once")
    eng.close()


def test_streamed_chunks(tmp_path, crafted):
    from numamma_amd.engine import Engine

    rp = crafted.rp
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.stream_begin(chunk_bytes=1 << 20)
    for r, a, data in rp.linear_buffers():
        eng.submit_buffer(data, r, a)
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    assert eng.route_count() >= 2
    _check_objects(eng, crafted, PRIMARY)
    _check_sites(eng, crafted, PRIMARY, tmp_path / "out")
    eng.close()


def _ent_objs(ent4):
    objs = np.zeros(ent4.shape[0], dtype=[("a", "<u8"), ("s", "<u8"), ("al", "<u8"), ("fr", "<u8")])
    objs["a"], objs["s"], objs["al"], objs["fr"] = ent4[:, 0], ent4[:, 1], ent4[:, 2], ent4[:, 3]
    return objs


def test_recorded_online_run(tmp_path):
    """Alarm tables listing subsets of the final table's ids; the site ids are
    those of the online report (every object reaches update_call_sites)."""
    from numamma_amd.engine import Engine, table_objects

    rp = generate(SynthConfig(nb_samples=120_000, nb_intervals=2_000, nb_threads=4, with_stack=False, reuse_frac=0.2,
                              buffer_records=500, seed=72))
    rp.buffers.reverse()  # online: oldest ring first
    t = rp.table
    snaps = [(be,) + table_at(t, ts) for be, ts in online_alarms(rp, 5)]
    c = Case(rp, str(tmp_path / "oracle"), alarms=snaps)
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
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
    assert eng.route_count() > 0
    o = px.Opts(2, (0, 1, 1, 0), 2)
    _check_objects(eng, c, o)
    _check_sites(eng, c, o, tmp_path / "out", online=True)
    h = str(tmp_path / "host")
    report_placement_host(_downloaded(eng, rp), t, h, online=True, **o.kw())
    assert _read(h) == _read(str(tmp_path / "out"))
    eng.close()


def test_two_workers_on_one_device(tmp_path, crafted):
    single = _run(crafted.rp)
    _check_sites(single, crafted, PRIMARY, tmp_path / "single")
    single.close()
    multi = _run(crafted.rp, devices=[0, 0])
    _check_objects(multi, crafted, PRIMARY)
    _check_sites(multi, crafted, PRIMARY, tmp_path / "multi")
    multi.close()
    assert _read(str(tmp_path / "multi")) == _read(str(tmp_path / "single"))


def test_run_replay_writes_blocks(tmp_path, crafted, monkeypatch):
    from numamma_amd.engine import run_replay

    path = str(tmp_path / "replay.bin")
    crafted.rp.write(path)
    d = str(tmp_path / "out")
    monkeypatch.delenv("NMG_REPLAY_PLACEMENT", raising=False)
    run_replay(path, d, str(tmp_path / "e.txt"))
    assert not os.path.exists(os.path.join(d, "blocks.dat"))
    monkeypatch.setenv("NMG_REPLAY_PLACEMENT", "2")
    run_replay(path, d, str(tmp_path / "e.txt"))
    assert _read(d) == px.expected_file(crafted.odir, crafted.rp.table, px.Opts(2, None, 8))
    monkeypatch.setenv("NMG_REPLAY_PLACEMENT", "4:0")
    run_replay(path, d, str(tmp_path / "e.txt"))
    assert _read(d) == px.expected_file(crafted.odir, crafted.rp.table, px.Opts(4, None, 0))


# ---- 3. errors

def test_rejections(tmp_path, small):
    from numamma_amd.engine import Engine, build_meta

    rp = small.rp  # 4 threads
    d = str(tmp_path / "out")

    def code(fn):
        with pytest.raises(_lib.NmgError) as ei:
            fn()
        return ei.value.code

    po, _ = _lib.placement_options(rp.nb_threads, 2)
    assert _lib.lib.nmg_count_object_blocks(None, po) == -1
    assert _lib.lib.nmg_get_object_blocks(None, po, None, 0) == -1
    assert _lib.lib.nmg_report_placement(None, None, None, po) == -1
    eng = Engine(flags=_lib.NMG_F_DEFAULT, nb_threads=rp.nb_threads)
    assert _lib.lib.nmg_count_object_blocks(eng.h, None) == -1
    assert code(lambda: eng.object_blocks(2)) == -6  # before nmg_set_objects
    eng.set_objects(rp.table)
    assert code(lambda: eng.report_placement(d, 0)) == -1 and code(lambda: eng.object_blocks(0)) == -1
    bad = [dict(nb_nodes=65), dict(nb_nodes=3), dict(nb_nodes=2, thread_node=[0, 1, 2, 0])]
    for kw in bad:
        assert code(lambda: eng.object_blocks(**kw)) == -1, kw
        assert code(lambda: eng.report_placement(d, **kw)) == -1, kw
    res1, _ = _lib.placement_options(rp.nb_threads, 2, reserved=1)  # non-zero reserved
    assert _lib.lib.nmg_count_object_blocks(eng.h, res1) == -1
    meta, keep = build_meta(rp.table)
    ro = _lib.nmg_report_options(d.encode(), 1, 0, None, None, None, 0, 0)
    assert _lib.lib.nmg_report_placement(eng.h, meta, ro, res1) == -1
    for short in ([0, 1], [0, 1, 0, 1, 0]):  # the binding: one node per thread rank
        with pytest.raises(ValueError):
            eng.object_blocks(2, thread_node=short)
        with pytest.raises(ValueError):
            eng.report_placement(d, 2, thread_node=short)
    assert not os.path.exists(d)
    eng.submit_replay(rp)
    eng.analyze()
    n = _lib.lib.nmg_count_object_blocks(eng.h, po)
    assert n > 0 and _lib.lib.nmg_get_object_blocks(eng.h, po, None, n) == -1  # rows NULL
    rows = np.zeros((n + 1, 5), dtype=np.uint64)
    assert _lib.lib.nmg_get_object_blocks(eng.h, po, rows.ctypes.data_as(_lib.u64p), n + 1) == -1  # the wrong count
    assert eng.object_blocks(64, thread_node=[63, 0, 63, 5]).shape[0] > 0  # the limits themselves
    assert eng.object_blocks(3, thread_node=[0, 1, 2, 2]).shape[0] > 0
    assert code(lambda: eng.report_placement("/nonexistent/dir", 2)) == -10  # NMG_ERR_IO
    eng.close()
    for flags in (_lib.NMG_F_MATCH_SAMPLES, _lib.NMG_F_PAGE_HIST):
        e2 = Engine(flags=flags, nb_threads=rp.nb_threads)
        e2.set_objects(rp.table)
        assert code(lambda: e2.object_blocks(2)) == -1
        assert code(lambda: e2.report_placement(d, 2)) == -1
        e2.close()
