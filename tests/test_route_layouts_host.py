"""The replays of route_layout_cases.py, checked on the host: that each one
has the compact-record layout it is named for, that stretching a profile's
dates by 256 changes nothing the oracle computes, that the multi-threaded
restatement agrees with the oracle on the saturation edge, and that the
cases hold what test_gpu_route_layouts.py relies on (so that its comparisons
cannot pass on an empty set)."""
import os

import numpy as np
import pytest

import pyoracle
import route_layout_cases as rc
from numamma_amd.replay import generate
from numamma_amd.results import RawResults

NO_MATCH = np.uint64(0xFFFFFFFFFFFFFFFF)


def _oracle(rp, d, tag):
    path = os.path.join(d, f"{tag}.bin")
    rp.write(path)
    raw = os.path.join(d, f"{tag}_raw.bin")
    pyoracle.run(path, os.path.join(d, f"{tag}_o"), os.path.join(d, f"{tag}.txt"), raw)
    return path, raw


@pytest.mark.parametrize("row", list(rc.LAYOUT_TABLE), ids=[f"T{t}-{n}buf" for t, n, _ in rc.LAYOUT_TABLE])
def test_layout_rows(row):
    T, nbuf, big = row
    rp, lay, planted = rc.layout_case(T, nbuf, big, split=1 if nbuf == 513 else 0)
    assert (lay["gbits"], lay["obits"], lay["tbits"], lay["loc"], lay["wbits"]) == rc.LAYOUT_TABLE[row]
    assert rp.nb_records() == 60_000 and len(rp.buffers) == nbuf
    ranks = {b.thread_rank for b in rp.buffers}
    assert max(ranks) == T - 1 and min(ranks) == 0
    # each planted weight on at least 100 samples the oracle matches
    rec = np.concatenate(rc.records(rp))
    for v, idx in planted:
        assert (rec["weight"][idx] == v).all()
        hit = rc.lookup_all(rp.table, rec["addr"][idx], rec["timestamp"][idx]) >= 0
        assert hit.sum() >= 100, (v, int(hit.sum()))


def test_cutover_cuts_hold_the_same_records(tmp_path):
    """512 and 513 buffers: the same records with the same threads, accesses and
    weights, so the oracle's per-object counters and page cells are equal."""
    a, la, _ = rc.layout_case(1024, 512)
    b, lb, _ = rc.layout_case(1024, 513, split=1)
    assert la["wbits"] == 11 and lb["wbits"] is None and lb["loc"] == 38
    assert np.array_equal(np.concatenate(rc.records(a)), np.concatenate(rc.records(b)))
    d = str(tmp_path)
    ra, rb = (RawResults.read(_oracle(rp, d, tag)[1]) for rp, tag in ((a, "a"), (b, "b")))
    assert ra.nb_found == rb.nb_found > 40_000
    assert np.array_equal(ra.count_weight, rb.count_weight) and np.array_equal(ra.cells, rb.cells)


@pytest.fixture(scope="module")
def long_run():
    base = generate(rc.STRETCH_CFG)
    return base, rc.stretch(base)


def test_stretch_moves_the_profile_past_the_time_field(long_run):
    base, st = long_run
    edge = rc.tbase_of(st.table) + (1 << rc.TS_BITS)
    ts = np.concatenate([r["timestamp"] for r in rc.records(st)])
    late = float((ts >= edge).mean())
    print(f"samples at or past tbase + 2^40: {late:.3f}")
    assert late >= 0.30
    ent = st.table.entries
    assert int((ent["alloc_date"] >= edge).sum()) >= 500
    assert int(((ent["alloc_date"] < edge) & (ent["free_date"] >= edge) & (ent["alloc_date"] != 0)).sum()) >= 500
    assert rc.tbase_of(st.table) == rc.T0 + (rc.tbase_of(base.table) - rc.T0) * rc.FACTOR


def test_stretch_invariance_on_the_oracle(long_run, tmp_path):
    d = str(tmp_path)
    a, b = (RawResults.read(_oracle(rp, d, tag)[1]) for rp, tag in zip(long_run, ("base", "stretched")))
    assert a.nb_found == b.nb_found > 40_000 and a.nb_samples == b.nb_samples == 60_000
    assert np.array_equal(a.global_counters, b.global_counters)
    assert np.array_equal(a.buf_samples, b.buf_samples) and np.array_equal(a.buf_found, b.buf_found)
    assert np.array_equal(a.count_weight, b.count_weight)
    assert np.array_equal(a.cells, b.cells)
    assert np.array_equal(a.first_ordinal != NO_MATCH, b.first_ordinal != NO_MATCH)
    assert np.array_equal(a.entries[:, 1:], b.entries[:, 1:])  # (the level buckets too)


@pytest.mark.parametrize("threads", [1, 5])
def test_mt_restatement_on_the_saturation_edge(long_run, tmp_path, threads):
    rp, _, _, _ = rc.edge_probes(long_run[1])
    d = str(tmp_path)
    path, raw = _oracle(rp, d, "probes")
    pyoracle.run_mt(path, os.path.join(d, "m_raw.bin"), threads=threads)
    assert open(raw, "rb").read() == open(os.path.join(d, "m_raw.bin"), "rb").read()


def test_edge_probes_decide_both_ways(long_run):
    rp, edge, edits, who = rc.edge_probes(long_run[1])
    assert edge == rc.tbase_of(rp.table) + (1 << 40) and len(edits) == 12  # eight single entries, four older ones
    eo = rp.table.entry_off
    assert sum(1 for pe, _, _ in edits if pe not in eo) == 4  # (not a key's newest entry)
    ent = rp.table.entries
    for pe, field, date in edits:
        assert int(ent[field][pe]) == date and ent["alloc_date"][pe] <= ent["free_date"][pe]
    probe = rc.records(rp)[-1]
    assert probe.shape[0] == who.shape[0] >= 12 * 3 * 7
    hit = rc.lookup_all(rp.table, probe["addr"], probe["timestamp"])
    for i, (pe, _, _) in enumerate(edits):
        mine = hit[who == i]
        assert ((mine == pe) | (mine == -1)).all()
        assert (mine == pe).any() and (mine == -1).any()
    # both sides of the quantum that saturates: a sample one quantum before the
    # edge still fits the record, a sample on it escapes
    rel = probe["timestamp"].astype(np.int64) - rc.tbase_of(rp.table)
    assert ((rel >> rc.Q_SHIFT) == 0xFFFFFFFE).any() and ((rel >> rc.Q_SHIFT) == 0xFFFFFFFF).any()
    assert (rel >> rc.TS_BITS != 0).any()


def test_narrow_long_run_case():
    """The long run at 1024 threads and 257 buffers (the probe buffer among
    them): wbits 11, and still mostly past the time field."""
    rp = rc.narrow_long_run()
    lay = rc.expected_layout(rp)
    assert (lay["gbits"], lay["obits"], lay["tbits"], lay["loc"], lay["wbits"]) == (9, 17, 10, 37, 11)
    ts = np.concatenate([r["timestamp"] for r in rc.records(rp)])
    assert float((ts >= lay["tbase"] + (1 << rc.TS_BITS)).mean()) >= 0.30
