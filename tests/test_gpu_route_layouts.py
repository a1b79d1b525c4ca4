"""The partition-first path over the compact record's whole layout space and
over a long run's dates (nmg_route.h XLayout; cases: route_layout_cases.py).

The 16-byte record route2_kernel hands to local_kernel and found_kernel has
run-time field widths: gbits (buffers), obits (longest buffer / 8), tbits
(threads), and wbits = min(48 - (gbits + obits + tbits + 1), 16) for the
weight; past gbits + obits + tbits + 1 = 37 the engine keeps
attribute_kernel.  The other GPU tests stay at wbits 16 with slack.  Here
60,000 records are re-cut so that wbits runs from 16 (with slack, and with
none: the thread field touches the location) down to 11, tbits from 0 to 10,
gbits from 2 to 11, with weights planted on both sides of each case's escape
mark, and every case asserts the layout the engine used (route_layout()).

The long run stretches a profile's dates by 256: 57 % of the samples lie more
than 2^40 ns after the table's first allocation and escape, the packed node
records' quantised dates saturate, and twelve entries (four of them older
entries of reused keys) have a date within a
quantum of that edge with probe samples around it.

The reference is the oracle's raw dump, compared as
tests/test_gpu_pool_pieces.py does: global and per-buffer counters (the found
counts come from found_kernel's gshift), object counters, levels, page cells."""
import dataclasses
import functools
import os

import numpy as np
import pytest

import cost_expect as cx
import pyoracle
import route_layout_cases as rc
import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd.replay import T0, Replay, generate
from numamma_amd.results import RawResults

pytestmark = pytest.mark.gpu

TINY_POOL = 0x20000     # (internal) private pools of two chunks: the overflow list, overflow_kernel
TINY_OVF = 0x80000      # (internal, with TINY_POOL) an overflow list of 64 records
NO_LINES = 0x20000000   # (internal) route pass without the LDS line stage
LEVELS = _lib.NMG_F_DEFAULT | _lib.NMG_F_OBJECT_LEVELS
DUMPS = LEVELS | _lib.NMG_F_SAMPLE_MATCHES
VARIANTS = {"route": 0, "tinyovf": TINY_POOL | TINY_OVF, "nolines": NO_LINES}
MAPS = ("00400000-00452000 r-xp 00000000 08:02 173521 /usr/bin/app\n"
        "555500000000-555600000000 rw-p 00000000 00:00 0 [heap]\n")

MATRIX = [(1024, n, rc.BIG) for n in (4, 9, 17, 33, 65, 129, 257, 512)] + \
         [(65, 2048, 1 << 19), (3, 5, rc.BIG), (1, 5, rc.BIG)]
# wbits 11, and wbits 16 with no slack
EDGE_ROWS = [(1024, 9, rc.BIG), (1024, 257, rc.BIG), (1024, 512, rc.BIG)]


def _id(row):
    return f"T{row[0]}-{row[1]}buf"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("layouts"))


def _oracle(rp, d, tag):
    path = os.path.join(d, f"{tag}.bin")
    rp.write(path)
    pyoracle.run(path, os.path.join(d, f"{tag}_o"), os.path.join(d, f"{tag}.txt"), os.path.join(d, f"{tag}_raw.bin"))
    os.remove(path)
    raw = RawResults.read(os.path.join(d, f"{tag}_raw.bin"))
    assert raw.nb_found > 40_000 and raw.cells.shape[0] > 0
    return raw


@pytest.fixture(scope="module")
def case_of(workdir):
    """(replay, expected layout, the oracle's results) of a layout row, built once."""
    @functools.lru_cache(maxsize=None)
    def get(row, split=0):
        rp, lay, _ = rc.layout_case(*row, split=split)
        assert (lay["gbits"], lay["obits"], lay["tbits"], lay["loc"], lay["wbits"]) == rc.LAYOUT_TABLE[row]
        return rp, lay, _oracle(rp, workdir, _id(row))
    return get


def _results(eng, levels=True):
    g, ns, nf = eng.global_counters()
    s, f = eng.buffer_counts()
    first, cw = eng.object_counters()
    return g, (ns, nf), s, f, first, cw, eng.object_levels() if levels else None, eng.page_cells().copy()


def _check(eng, raw, levels=True):
    g, nsf, s, f, first, cw, lv, cells = _results(eng, levels)
    assert np.array_equal(g, raw.global_counters) and nsf == (raw.nb_samples, raw.nb_found)
    assert np.array_equal(s, raw.buf_samples) and np.array_equal(f, raw.buf_found)
    assert np.array_equal(first, raw.first_ordinal)
    assert np.array_equal(cw, raw.count_weight)
    if levels:
        assert np.array_equal(lv, cx.oracle_levels(raw))
    assert np.array_equal(cells, raw.cells)
    return f, cw, cells


def _engine(rp, flags):
    from numamma_amd.engine import Engine

    eng = Engine(flags=flags, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    return eng


def _analyze(rp, flags):
    eng = _engine(rp, flags)
    eng.submit_replay(rp)
    eng.analyze()
    eng.synchronize()
    return eng


def _used(eng, lay):
    """The engine took the partition-first path with the layout the case is named for."""
    assert eng.route_count() > 0
    got = eng.route_layout()
    print("route_layout", got)
    assert got == {k: lay[k] for k in got}


@pytest.mark.parametrize("row", MATRIX, ids=_id)
def test_layout_matrix(case_of, row):
    rp, lay, raw = case_of(row)
    eng = _analyze(rp, LEVELS)
    _used(eng, lay)
    _check(eng, raw)
    eng.close()


@pytest.mark.parametrize("variant", ["tinyovf", "nolines"])
@pytest.mark.parametrize("row", EDGE_ROWS, ids=_id)
def test_edge_layouts_other_paths(case_of, row, variant):
    """overflow_kernel and the route pass without its line stage decode the same words."""
    rp, lay, raw = case_of(row)
    eng = _analyze(rp, LEVELS | VARIANTS[variant])
    _used(eng, lay)
    _check(eng, raw)
    eng.close()


@pytest.mark.parametrize("row", EDGE_ROWS, ids=_id)
def test_edge_layouts_dump_modes(case_of, workdir, row):
    """NMG_F_SAMPLE_MATCHES: the per-sample matches and the dump files, which
    re-read every raw record through the word's buffer index and offset."""
    rp, lay, _ = case_of(row)
    d = os.path.join(workdir, "dump_" + _id(row))
    os.makedirs(d)
    path = os.path.join(d, "replay.bin")
    rp.write(path)
    odir, edir = os.path.join(d, "oracle"), os.path.join(d, "engine")
    pyoracle.run(path, odir, os.path.join(d, "o.txt"), dump=True, dump_all=True, dump_unmatched=True,
                 maps_path="/proc/4242/maps", maps_text=MAPS)
    os.remove(path)
    eng = _analyze(rp, DUMPS)
    _used(eng, lay)
    eng.report(edir, os.path.join(d, "e.txt"), dump_flags=_lib.NMG_DUMP_CALLSITES | _lib.NMG_DUMP_ALL | _lib.NMG_DUMP_UNMATCHED,
               maps_path="/proc/4242/maps", maps_text=MAPS)
    eng.close()
    assert open(os.path.join(d, "o.txt"), "rb").read() == open(os.path.join(d, "e.txt"), "rb").read()
    names = sorted(os.listdir(odir))
    assert names == sorted(os.listdir(edir)) and "all_memory_accesses.dat" in names and "unmatched_samples.log" in names
    for n in names:
        assert open(os.path.join(odir, n), "rb").read() == open(os.path.join(edir, n), "rb").read(), n


def test_cutover_to_single_pass(case_of):
    """513 buffers at 1024 threads: one location bit too many, no route launch,
    and the results of the 512-buffer cut (the same records, threads, weights)."""
    rp, lay, raw = case_of((1024, 513, rc.BIG), 1)
    assert lay["loc"] == 38 and lay["wbits"] is None
    eng = _analyze(rp, LEVELS)
    assert eng.route_count() == 0 and not any(eng.route_layout().values())
    _, cw, cells = _check(eng, raw)
    eng.close()
    rp2, lay2, raw2 = case_of((1024, 512, rc.BIG))
    eng = _analyze(rp2, LEVELS)
    _used(eng, lay2)
    _, cw2, cells2 = _check(eng, raw2)
    eng.close()
    assert np.array_equal(cw, cw2) and np.array_equal(cells, cells2)


def _stream(eng, rp, cut):
    """rp's buffers as two streamed chunks, the first ending after `cut`
    buffers; the layout of each chunk's launch."""
    eng.stream_begin(chunk_bytes=64 << 20, copy_threads=2)
    lays = []
    for i, (r, a, data) in enumerate(rp.linear_buffers()):
        eng.submit_buffer(data, r, a)
        if i + 1 == cut:
            eng.analyze()
            lays.append(eng.route_layout())
    eng.analyze()
    eng.stream_end()
    lays.append(eng.route_layout())
    eng.synchronize()
    return lays


def test_layout_changes_between_chunks(case_of, workdir):
    """One engine, two streamed chunks: 4 buffers (wbits 16), then 300 buffers
    of a second sample stream over the same table (wbits 11), each chunk's
    found counts decoded with its own gshift; then a reset and both again."""
    first, _, _ = case_of((1024, 4, rc.BIG))
    more = generate(dataclasses.replace(rc.LAYOUT_CFG, sample_seed=77))
    assert np.array_equal(more.table.entries, first.table.entries)
    second = rc.recut(more, 1024, 300, rc.BIG, seed=1300)
    rc.plant_weights(second, 2047, seed=300)
    rp = Replay(1024, first.table, first.buffers + second.buffers)
    raw = _oracle(rp, workdir, "two_chunks")
    want = [rc.expected_layout(first), rc.expected_layout(second)]
    assert [w["wbits"] for w in want] == [16, 11] and [w["gbits"] for w in want] == [2, 9]
    eng = _engine(rp, LEVELS)
    for launches in (2, 4):
        lays = _stream(eng, rp, 4)
        assert eng.route_count() == launches
        assert lays[0] != lays[1]
        for got, w in zip(lays, want):
            assert got == {k: w[k] for k in got}
        _check(eng, raw)
        eng.reset()
        eng.clear_buffers()
    eng.close()


# ---- long runs

LONG_VARIANTS = {"route": 0, "tinypool": TINY_POOL, "nolines": NO_LINES, "single": _lib.NMG_F_SINGLE_PASS}


@pytest.fixture(scope="module")
def long_run(workdir):
    base = generate(rc.STRETCH_CFG)
    st = rc.stretch(base)
    probes, edge, _, _ = rc.edge_probes(st)
    late = np.concatenate([r["timestamp"] for r in rc.records(st)]) >= edge
    assert late.mean() >= 0.30
    return {"base": (base, _oracle(base, workdir, "long_base")), "stretched": (st, _oracle(st, workdir, "long_st")),
            "probes": (probes, _oracle(probes, workdir, "long_probes"))}


@pytest.mark.parametrize("variant", list(LONG_VARIANTS))
def test_long_run(long_run, variant):
    """Dates up to 2^41 ns past tbase: every run equals the oracle, and the
    stretched replay gives what the unstretched one gives."""
    flags = LEVELS | LONG_VARIANTS[variant]
    out = {}
    for name, (rp, raw) in long_run.items():
        eng = _analyze(rp, flags)
        if variant == "single":  # (NMG_F_SINGLE_PASS asks for attribute_kernel)
            assert eng.route_count() == 0
        else:
            lay = rc.expected_layout(rp)
            assert lay["wbits"] == 16
            _used(eng, lay)
            assert eng.route_layout()["tbase"] == rc.tbase_of(rp.table)
        out[name] = _check(eng, raw)
        eng.close()
    for x, y in zip(out["base"], out["stretched"]):  # buf_found, count_weight, page cells
        assert np.array_equal(x, y)


@pytest.mark.parametrize("variant", ["route", "tinyovf"])
def test_long_run_narrow_layout(workdir, variant):
    """The long run at 1024 threads and 257 buffers: every late record escapes
    through a word with an 11-bit weight field."""
    rp = rc.narrow_long_run()
    raw = _oracle(rp, workdir, "narrow_" + variant)
    lay = rc.expected_layout(rp)
    assert lay["wbits"] == 11 and lay["loc"] == 37
    eng = _analyze(rp, LEVELS | VARIANTS[variant])
    _used(eng, lay)
    _check(eng, raw)
    eng.close()


# ---- timeline and cost cells at wide thread counts

@pytest.mark.parametrize("T", [65, 1024])
def test_timeline_and_cost_cells_wide_threads(workdir, T):
    rp = rc.recut(rc.base_replay(), T, 4, rc.BIG, seed=2000 + T)
    rc.plant_weights(rp, 65535, seed=T)
    raw, odir = tx.run_oracle(rp, os.path.join(workdir, f"wide{T}"))
    o = tx.TlOpts(t0=T0 + (1 << 31), bin_shift=31, nb_bins=4, min_object_bytes=8192)
    want_tl, _ = tx.expected_rows(odir, rp.table, T, o)
    want_cost, picked = cx.Dump(odir, rp.table, T).rows(cx.MEMORY_WEIGHT)
    assert set(np.unique(want_tl[:, 1]).tolist()) == {0, 1, 2, 3} and int(want_tl[:, 2].max()) == T - 1
    assert picked > 1000 and int(want_cost[:, 1].max()) == T - 1
    eng = _engine(rp, LEVELS)
    eng.set_timeline(**o.kw())
    eng.set_page_cost(**cx.MEMORY_WEIGHT.kw())
    eng.submit_replay(rp)
    eng.analyze()
    eng.synchronize()
    _used(eng, rc.expected_layout(rp))
    _check(eng, raw)
    assert np.array_equal(eng.timeline_cells(), want_tl)
    assert np.array_equal(eng.cost_cells(), want_cost)
    eng.close()
