"""The engine against what the reference's own sample loop returned.

tests/golden/ref_loop/<case>_<size>.npz holds the results of the reference's
src/mem_sampling.c + src/mem_analyzer.c (compiled unchanged; see
test_reference_loop.py, which regenerates and compares the files) on three
replays that ref_loop_cases.py rebuilds here: every mem_lvl value once per
access type (sweep), the irregular record streams (streams) and the lookup
boundaries (edges).  The kernels are compared with those vectors directly,
not through the oracle's restatement, on every path that counts levels or
looks objects up: attribute_kernel (40 keys), route + local (1040 keys), the
pool-overflow list and in-route attribution (internal switches 0x20000,
0x20000 | 0x80000), NMG_F_SINGLE_PASS on the large table; batch and streamed
in 64 KiB chunks; with NMG_F_OBJECT_LEVELS the per-object level rows; with
page cost cells, sums derived from the recorded per-object counters.

Every comparison is exact equality.  Nothing here reads the reference."""
import numpy as np
import pytest

import cost_expect as cx
import ref_loop_cases as rc
from numamma_amd import _lib

pytestmark = pytest.mark.gpu

TINY_POOL = 0x20000  # (internal) private pools of two chunks: the overflow list, overflow_kernel
TINY_OVF = 0x80000   # (internal, with TINY_POOL) an overflow list of 64 records: the rest attributed in the route pass
LEVELS = _lib.NMG_F_OBJECT_LEVELS
SINGLE = _lib.NMG_F_SINGLE_PASS

# (id, table size, extra flags, streamed)
PATHS = [
    ("attribute-batch", "small", 0, False),
    ("attribute-stream", "small", 0, True),
    ("attribute-levels", "small", LEVELS, False),
    ("route-batch", "large", 0, False),
    ("route-stream", "large", 0, True),
    ("route-levels", "large", LEVELS, False),
    ("route-levels-stream", "large", LEVELS, True),
    ("tinypool", "large", TINY_POOL, False),
    ("tinypool-levels", "large", TINY_POOL | LEVELS, False),
    ("tinyovf-levels", "large", TINY_POOL | TINY_OVF | LEVELS, False),
    ("single-pass", "large", SINGLE, False),
    ("single-pass-levels", "large", SINGLE | LEVELS, False),
]


@pytest.fixture(scope="module")
def golden():
    out = {}
    for case in rc.CASES:
        for size in rc.SIZES:
            g = rc.load_golden(case, size)
            for v in g.values():
                v.setflags(write=False)
            out[case, size] = g
    return out


def _run(rp, flags, streamed=False, before=None):
    from numamma_amd.engine import Engine

    eng = Engine(flags=_lib.NMG_F_DEFAULT | flags, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    if before:
        before(eng)
    if streamed:
        eng.stream_begin(chunk_bytes=64 << 10)
    eng.submit_replay(rp)
    eng.analyze()
    if streamed:
        eng.stream_end()
    eng.synchronize()
    return eng


def _routes(eng, size, flags):
    """The kernel the table size and the flags ask for did the work."""
    return eng.route_count() > 0 if size == "large" and not flags & SINGLE else eng.route_count() == 0


def _check(eng, g, levels):
    glob, ns, nf = eng.global_counters()
    assert np.array_equal(glob, g["global"])  # minima and maxima included
    assert (ns, nf) == (int(g["totals"][0]), int(g["totals"][1]))
    s, f = eng.buffer_counts()
    assert np.array_equal(s, g["buf_samples"]) and np.array_equal(f, g["buf_found"])
    ent = g["entries"].reshape(-1, 2, rc.SUM_WORDS)
    _, cw = eng.object_counters()
    assert np.array_equal(cw, ent[:, :, :2])
    assert np.array_equal(eng.page_cells(), g["cells"])
    if levels:
        assert np.array_equal(eng.object_levels(), ent[:, :, 2:])


@pytest.mark.parametrize("case", list(rc.CASES))
@pytest.mark.parametrize("name,size,flags,streamed", PATHS, ids=[p[0] for p in PATHS])
def test_engine_equals_reference_vectors(golden, case, name, size, flags, streamed):
    rp = rc.replay(case, size)
    eng = _run(rp, flags, streamed)
    assert _routes(eng, size, flags)
    _check(eng, golden[case, size], bool(flags & LEVELS))
    eng.close()


def _cost_sums(eng, rp):
    """The cost cells summed per entry (u64, wrapping), and the entries that have such cells."""
    rows = eng.cost_cells()
    cells = eng.page_cells()
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(42)) | (r[:, 1].astype(np.uint64) << np.uint64(32)) \
        | r[:, 2].astype(np.uint64)  # noqa: E731
    assert np.isin(key(rows), key(cells)).all()  # a cost cell lies on a counted page
    return cx.entry_sums(rows, rp.table.nb_entries), cx.dense(rp.table, rp.nb_threads)


@pytest.mark.parametrize("size,flags", [("small", 0), ("large", 0), ("large", TINY_POOL), ("large", SINGLE)],
                         ids=["attribute", "route", "tinypool", "single-pass"])
def test_memory_cost_by_weight_equals_recorded_sums(golden, size, flags):
    """NMG_COST_MEMORY by weight on the irregular streams, whose samples carry
    one level each (or none): a sample is selected by at most one of the three
    buckets, so an entry's cells add up to the recorded weight sums of local
    RAM hit + remote RAM hit + remote cache hit over both access types."""
    rp, g = rc.replay("streams", size), golden["streams", size]
    eng = _run(rp, flags, before=lambda e: e.set_page_cost(_lib.NMG_COST_MEMORY, 3, _lib.NMG_COST_WEIGHT))
    assert _routes(eng, size, flags)
    _check(eng, g, False)
    got, dense = _cost_sums(eng, rp)
    ent = g["entries"].reshape(-1, 2, rc.SUM_WORDS)
    want = np.zeros(rp.table.nb_entries, dtype=np.uint64)
    for b in (4, 5, 6):
        want += ent[:, 0, 3 + 2 * b + 1] + ent[:, 1, 3 + 2 * b + 1]
    assert dense.sum() >= 39 and want[dense].any()
    assert np.array_equal(got[dense], want[dense]) and not got[~dense].any()
    eng.close()


@pytest.mark.parametrize("bucket", [4, 5, 6, 14], ids=["local-ram-hit", "remote-ram-hit", "remote-cache-hit",
                                                        "remote-ram-miss"])
@pytest.mark.parametrize("size", rc.SIZES)
def test_level_sweep_cost_per_bucket(golden, size, bucket):
    """One bucket of NMG_COST_MEMORY at a time (and a merged miss bucket) on
    the level sweep, where a sample sits in up to nine buckets: by weight, an
    entry's cells add up to that bucket's recorded weight sum (u64, wrapping:
    the sweep carries weights up to 2^63)."""
    rp, g = rc.replay("sweep", size), golden["sweep", size]
    eng = _run(rp, 0, before=lambda e: e.set_page_cost(1 << bucket, 3, _lib.NMG_COST_WEIGHT))
    assert _routes(eng, size, 0)
    got, dense = _cost_sums(eng, rp)
    ent = g["entries"].reshape(-1, 2, rc.SUM_WORDS)
    want = ent[:, 0, 3 + 2 * bucket + 1] + ent[:, 1, 3 + 2 * bucket + 1]
    assert dense.all() and np.count_nonzero(want) >= 60
    assert np.array_equal(got, want)
    eng.close()
