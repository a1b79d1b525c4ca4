"""The reference side of the irregular record streams (stream_grammar.py),
checked on the CPU before the kernels are held to it:

* the oracle's per-buffer SAMPLE counts equal the independent byte cursor's;
* the oracle gives the same counters, page cells, stdout (but for the bytes
  processed) and report files for an irregular replay and for its normalised
  twin -- the same samples re-emitted as pure 40 B records, a stream every
  other test already trusts the oracle on;
* the multi-threaded restatement (a third parser) equals the oracle;
* the replay file round-trips;
* every pattern that holds samples contributes matched ones, and gives a
  parser without the slow path or without the type test another count."""
import os

import numpy as np
import pytest

import pyoracle
import stream_grammar as sg
from numamma_amd.replay import Replay
from numamma_amd.results import RawResults


def _run(rp, d, tag):
    path = os.path.join(d, tag + ".bin")
    rp.write(path)
    odir = os.path.join(d, tag)
    pyoracle.run(path, odir, os.path.join(d, tag + ".txt"), os.path.join(d, tag + "_raw.bin"))
    return path, odir, RawResults.read(os.path.join(d, tag + "_raw.bin"))


def _stdout_without_bytes(path):
    lines = open(path, "rb").read().split(b"\n")
    kept = [l for l in lines if b"bytes processed" not in l]
    assert len(kept) == len(lines) - 1  # exactly the one line
    return kept


@pytest.fixture(scope="module", params=[300, 3000])
def case(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp(f"grammar{request.param}"))
    rp = sg.grammar_replay(request.param)
    path, odir, raw = _run(rp, d, "irregular")
    return d, rp, path, odir, raw


def test_oracle_counts_equal_the_byte_cursor(case):
    d, rp, path, odir, raw = case
    want = []
    for _, _, lin in rp.linear_buffers():
        samples, err = sg.walk(lin)
        assert err is None
        want.append(len(samples))
    assert raw.buf_samples.tolist() == want
    assert raw.nb_samples == sum(want)
    tiny = sg.tiny_replay(int(rp.table.nb_keys) - 9, nb_buffers=16_384)
    _, _, traw = _run(tiny, d, "tiny")
    assert traw.buf_samples.tolist() == [len(sg.walk(lin)[0]) for _, _, lin in tiny.linear_buffers()]
    assert 2 * traw.nb_found >= traw.nb_samples > 16_384


def test_oracle_irregular_equals_normalised(case):
    d, rp, path, odir, raw = case
    _, ndir, nraw = _run(sg.normalised(rp), d, "normalised")
    assert np.array_equal(raw.global_counters, nraw.global_counters)
    assert (raw.nb_samples, raw.nb_found) == (nraw.nb_samples, nraw.nb_found)
    assert np.array_equal(raw.buf_samples, nraw.buf_samples) and np.array_equal(raw.buf_found, nraw.buf_found)
    assert np.array_equal(raw.count_weight, nraw.count_weight)
    assert np.array_equal(raw.entries[:, 1:], nraw.entries[:, 1:])  # (levels; word 0 holds the first ordinal's offset)
    assert np.array_equal(raw.cells, nraw.cells)
    # first-match ordinals: the same buffer, another byte offset
    assert np.array_equal(raw.first_ordinal >> np.uint64(32), nraw.first_ordinal >> np.uint64(32))
    assert _stdout_without_bytes(os.path.join(d, "irregular.txt")) == _stdout_without_bytes(os.path.join(d, "normalised.txt"))
    assert sorted(os.listdir(odir)) == sorted(os.listdir(ndir))
    for f in os.listdir(odir):
        assert open(os.path.join(odir, f), "rb").read() == open(os.path.join(ndir, f), "rb").read(), f


@pytest.mark.parametrize("threads", [1, 5])
def test_mt_restatement_equals_oracle(case, threads):
    d, rp, path, odir, raw = case
    mt = os.path.join(d, f"mt{threads}_raw.bin")
    t = pyoracle.run_mt(path, mt, threads=threads)
    assert t["nb_samples"] == raw.nb_samples
    assert open(os.path.join(d, "irregular_raw.bin"), "rb").read() == open(mt, "rb").read()


def test_replay_file_round_trip(case):
    d, rp, path, odir, raw = case
    back = Replay.read(path)
    assert back.nb_threads == rp.nb_threads and len(back.buffers) == len(rp.buffers)
    for a, b in zip(rp.buffers, back.buffers):
        assert (a.thread_rank, a.access_type, a.data_tail, a.data_head) == \
            (b.thread_rank, b.access_type, b.data_tail, b.data_head)
        assert np.array_equal(a.ring, b.ring)
    again = os.path.join(d, "again.bin")
    back.write(again)
    assert open(path, "rb").read() == open(again, "rb").read()


def _stride_parser(raw):
    """A wrong parser: every 40 B stride slot holding a SAMPLE header of size 40
    (a fast path taken without its whole-window check)."""
    n = raw.shape[0] // 40
    rec = raw[:40 * n].view(sg.RECORD_DTYPE)
    return int(((rec["type"] == sg.SAMPLE) & (rec["size"] == 40)).sum())


def _typeless_parser(raw):
    """A wrong parser: the right cursor, counting every record whose 40 B fit (no type test)."""
    data, cur, n = bytes(raw), 0, 0
    while cur + 8 <= len(data):
        size = int.from_bytes(data[cur + 6:cur + 8], "little")
        n += cur + 40 <= len(data)
        cur += size
    return n


def test_patterns_tell_wrong_parsers_apart(case):
    """Each pattern holding records gives a parser without the slow path, or
    one without the type test, another SAMPLE count than walk(): a kernel
    with that mistake cannot equal the oracle on it."""
    d, rp, path, odir, raw = case
    for name, (first, count) in rp.meta["patterns"].items():
        lins = [b.linear() for b in rp.buffers[first:first + count]]
        want = sum(len(sg.walk(x)[0]) for x in lins)
        stride = sum(_stride_parser(x) for x in lins)
        typeless = sum(_typeless_parser(x) for x in lins)
        if name == "empty":
            assert stride == typeless == want == 100
        elif name == "overshoot":  # a parser that takes every record past the end for truncated reports an error
            (lin,) = lins
            size = int.from_bytes(bytes(lin[2800 + 6:2800 + 8]), "little")
            assert want == 70 and sg.walk(lin)[1] is None and 2800 + size > lin.shape[0] >= 2808
        elif name in ("type40", "nosample"):
            assert typeless != want, name
        else:
            assert stride != want, name


def test_every_pattern_matches(case):
    d, rp, path, odir, raw = case
    kept = sg.kept_index(rp)
    assert set(rp.meta["patterns"]) == set(sg.PATTERNS)
    for name, (first, count) in rp.meta["patterns"].items():
        idx = [kept[i] for i in range(first, first + count) if kept[i] >= 0]
        found = int(raw.buf_found[idx].sum())
        if name == "nosample":
            assert int(raw.buf_samples[idx].sum()) == 0
        elif name == "empty":
            assert len(idx) == count - 1  # the empty ring is dropped, its neighbours stay
        else:
            assert found > 0, name
    # a parser that lost a pattern's samples would fall below this (measured: about 83 %)
    assert 2 * raw.nb_found >= raw.nb_samples
