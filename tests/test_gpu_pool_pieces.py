"""The route pass's chunk pool in pieces (numamma_amd/csrc/nmg_pool_layout.h).

The pool is a set of device allocations of 2^K chunks; a workgroup's private
chunk range lies in one of them; route2_kernel, scatter_kernel and
found_kernel find a workgroup's piece in the table of base pointers, and
local_kernel reads each chunk at the distance scatter_kernel noted.  With the
shipped piece size (64 MiB) a small workload has one piece, so these tests set
the internal switch 0x200000: the smallest pieces that hold the largest
workgroup pool.  The workload -- 3,000 intervals (three partitions or more),
60,000 records in 32 buffers of two sizes, one buffer per workgroup -- then
spans some twenty pieces, with ids skipped before a range that would cross a
piece boundary and several of the small ranges sharing a piece; the tests
assert that shape from the engine's own account of its pool (route_pool()).

The reference is the oracle's raw dump, compared as tests/test_gpu_route.py
and tests/test_gpu_route_levels.py do: global and per-buffer counters (the
found counts come from found_kernel), object counters, levels, page cells."""
import os

import numpy as np
import pytest

import pyoracle
from numamma_amd import _lib
from numamma_amd.replay import SynthConfig, generate
from numamma_amd.results import RawResults

pytestmark = pytest.mark.gpu

TINY_PIECES = 0x200000  # (internal) pool pieces as small as the largest workgroup pool allows
TINY_POOL = 0x20000     # (internal) private pools of two chunks: the overflow list, overflow_kernel
TINY_OVF = 0x80000      # (internal, with TINY_POOL) an overflow list of 64 records
NO_LINES = 0x20000000   # (internal) route pass without the LDS line stage
LEVELS = _lib.NMG_F_DEFAULT | _lib.NMG_F_OBJECT_LEVELS


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    rp = generate(SynthConfig(nb_samples=60_000, nb_intervals=3_000, buffer_records=2_300, seed=97))
    assert len(rp.buffers) >= 24 and rp.nb_threads == 8
    d = str(tmp_path_factory.mktemp("pieces"))
    path = os.path.join(d, "replay.bin")
    rp.write(path)
    pyoracle.run(path, os.path.join(d, "oracle"), os.path.join(d, "o.txt"), os.path.join(d, "o_raw.bin"))
    os.remove(path)
    raw = RawResults.read(os.path.join(d, "o_raw.bin"))
    assert raw.nb_found > 0 and raw.cells.shape[0] > 0
    return rp, raw


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
    ent = raw.entries
    if levels:
        assert np.array_equal(lv, np.stack([ent[:, 3:40], ent[:, 42:79]], axis=1))
    assert np.array_equal(cells, raw.cells)


def _analyze(rp, flags):
    from numamma_amd.engine import Engine

    eng = Engine(flags=flags, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.submit_replay(rp)
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() > 0
    return eng


@pytest.mark.parametrize("extra", [0, TINY_POOL | TINY_OVF, NO_LINES], ids=["route", "tinypool", "nolines"])
def test_tiny_pieces(case, extra):
    rp, raw = case
    eng = _analyze(rp, LEVELS | TINY_PIECES | extra)
    pool = eng.route_pool()
    assert pool["pieces"] >= 4
    if not extra & TINY_POOL:  # (pools of two chunks tile a piece: nothing to skip)
        assert pool["ids"] > pool["asked"]       # ids skipped before a piece boundary
        assert pool["pieces"] < len(rp.buffers)  # and more than one workgroup (= buffer) in some piece
    _check(eng, raw)
    eng.close()


def test_default_pieces_equal_tiny_pieces(case):
    rp, raw = case
    out = []
    for extra in (TINY_PIECES, 0):
        eng = _analyze(rp, _lib.NMG_F_DEFAULT | extra)
        out.append((eng.route_pool(), _results(eng, levels=False)))
        _check(eng, raw, levels=False)
        eng.close()
    (tiny, a), (default, b) = out
    assert tiny["pieces"] >= 4 and default["pieces"] == 1 and default["piece_log2"] == 16
    for x, y in zip(a, b):
        assert x is y or np.array_equal(x, y)


def _stream(eng, rp, cuts):
    """The buffers as streamed chunks that end after the buffers in `cuts`
    (analyze() enqueues the open chunk) and with the stream."""
    eng.stream_begin(chunk_bytes=64 << 20, copy_threads=2)
    pools = []
    for i, (r, a, data) in enumerate(rp.linear_buffers()):
        eng.submit_buffer(data, r, a)
        if i + 1 in cuts:
            eng.analyze()
            pools.append(eng.route_pool())
    eng.analyze()
    eng.stream_end()
    pools.append(eng.route_pool())
    eng.synchronize()
    return pools


def test_reuse_and_growth(case):
    """One engine, three streamed chunks, each larger than the one before, so
    that the pool is built anew with more pieces between launches; then a
    reset and the whole stream again on the pool the first pass left."""
    from numamma_amd.engine import Engine

    rp, raw = case
    eng = Engine(flags=LEVELS | TINY_PIECES, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    pools = _stream(eng, rp, (2, 14))
    assert eng.route_count() == 3
    assert pools[0]["pieces"] < pools[1]["pieces"] < pools[2]["pieces"]
    assert pools[0]["piece_log2"] < pools[1]["piece_log2"]
    _check(eng, raw)
    eng.reset()
    eng.clear_buffers()
    again = _stream(eng, rp, (2, 14))
    assert eng.route_count() == 6
    assert [p["bytes"] for p in again] == [pools[2]["bytes"]] * 3  # the pool is kept
    _check(eng, raw)
    eng.close()
