"""Per-object level counters (NMG_F_OBJECT_LEVELS) and the dump modes'
per-sample matches (NMG_F_SAMPLE_MATCHES) on the partition-first path.

Large tables (> 1023 keys) take route2_kernel + local_kernel with these flags
too; every test here drives Engine directly and asserts route_count() > 0, so
it checks the route kernels and not attribute_kernel (NMG_F_SINGLE_PASS is the
one variant that must report 0).  The reference is the oracle, whose raw dump
holds entry[E][ENTRY_WORDS] (numamma_amd/results.py): with G = GLOBAL_SUMS,
ent[:, 1 + G * a + 2 : 1 + G * a + G] is object_levels()[:, a, :] (na_miss,
then NB_BUCKETS x (count, sum)).

Sizes are the smallest that reach each mechanism: two or three partitions of
~100k records (several 1023-chunk work items per partition: the atomic flush),
the overflow list and the in-route direct attribution (internal switches
0x20000, 0x80000), escaped compact records, weights past the packed LDS
counters, streamed chunks, an online table's id map, two workers."""
import dataclasses
import os

import numpy as np
import pytest

import pyoracle
from numamma_amd import _lib
from numamma_amd.replay import (LVL_HIT, LVL_IO, LVL_L1, LVL_L2, LVL_L3, LVL_LFB, LVL_LOC_RAM, LVL_MISS, LVL_NA,
                                LVL_REM_CCE1, LVL_REM_CCE2, LVL_REM_RAM1, LVL_REM_RAM2, LVL_UNC, RECORD_DTYPE, T0,
                                SynthConfig, generate, online_alarms, table_at)
from numamma_amd.results import RawResults

pytestmark = pytest.mark.gpu

TINY_POOL = 0x20000    # (internal) private pools of two chunks: the overflow list, overflow_kernel
TINY_OVF = 0x80000     # (internal, with TINY_POOL) an overflow list of 64 records: the rest attributed in the route pass
NO_LINES = 0x20000000  # (internal) route pass without the LDS line stage
LEVELS = _lib.NMG_F_DEFAULT | _lib.NMG_F_OBJECT_LEVELS
DUMPS = LEVELS | _lib.NMG_F_SAMPLE_MATCHES
ROUTE_VARIANTS = [0, TINY_POOL, TINY_POOL | TINY_OVF, NO_LINES]
ROUTE_IDS = ["route", "tinypool", "tinyovf", "nolines"]


def _levels(raw):
    """The oracle's per-object levels as object_levels() lays them out."""
    ent = raw.entries
    return np.stack([ent[:, 3:40], ent[:, 42:79]], axis=1)


def _oracle(rp, d, **kw):
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "replay.bin")
    rp.write(path)
    pyoracle.run(path, os.path.join(d, "oracle"), os.path.join(d, "o.txt"), os.path.join(d, "o_raw.bin"), **kw)
    os.remove(path)
    return RawResults.read(os.path.join(d, "o_raw.bin"))


def _check_all(eng, raw, idmap=None):
    """Every counter of the engine against the oracle's raw dump: global, per
    buffer, object (first match, count, weight), levels, page cells.  idmap:
    the engine's entry id of each oracle entry (an online table)."""
    g, ns, nf = eng.global_counters()
    assert np.array_equal(g, raw.global_counters) and (ns, nf) == (raw.nb_samples, raw.nb_found)
    s, f = eng.buffer_counts()
    assert np.array_equal(s, raw.buf_samples) and np.array_equal(f, raw.buf_found)
    first, cw = eng.object_counters()
    lv = eng.object_levels()
    cells = eng.page_cells().copy()
    if idmap is not None:
        first, cw, lv = first[idmap], cw[idmap], lv[idmap]
        pos = np.empty_like(idmap)
        pos[idmap] = np.arange(idmap.shape[0], dtype=np.uint32)
        cells[:, 0] = pos[cells[:, 0]]
        cells = cells[np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))]
    assert np.array_equal(first, raw.first_ordinal)
    assert np.array_equal(cw, raw.count_weight)
    assert np.array_equal(lv, _levels(raw))
    assert np.array_equal(cells, raw.cells)


def _run_resident(rp, flags):
    """One analysis of rp's buffers, device-resident; the engine, synchronised."""
    import torch
    from numamma_amd.engine import Engine

    arena, offs, lens, ranks, acc = rp.packed()
    dev = torch.from_numpy(arena).cuda()
    eng = Engine(flags=flags, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.set_device_buffers(dev.data_ptr(), offs, lens, ranks, acc)
    eng.analyze()
    eng.synchronize()
    eng._arena = dev  # (the buffers live as long as the engine)
    return eng


def _samples(rp):
    """The buffers' records (pure 40 B SAMPLE streams: no LOST records, no wrap)."""
    return [b.ring.view(RECORD_DTYPE) for b in rp.buffers]


# ---- 1. level parity on the path

@pytest.fixture(scope="module")
def parity_case(tmp_path_factory):
    # two or three partitions of ~100k records: several work items per
    # partition, so the non-exclusive (atomic) flush runs; LOST records, one
    # wrapped ring
    rp = generate(SynthConfig(nb_samples=200_000, nb_intervals=2_000, lost_frac=1e-3, wrap_one=True, seed=91))
    raw = _oracle(rp, str(tmp_path_factory.mktemp("parity")))
    assert raw.nb_found > 0 and _levels(raw).sum() > 0
    return rp, raw


@pytest.mark.parametrize("extra", ROUTE_VARIANTS + [_lib.NMG_F_SINGLE_PASS], ids=ROUTE_IDS + ["single"])
def test_levels_parity_on_route_path(parity_case, extra):
    from numamma_amd.engine import Engine

    rp, raw = parity_case
    eng = Engine(flags=LEVELS | extra, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.submit_replay(rp)  # (staged: rings linearised by the engine, the wrapped one included)
    eng.analyze()
    eng.synchronize()
    assert (eng.route_count() == 0) if extra == _lib.NMG_F_SINGLE_PASS else (eng.route_count() > 0)
    _check_all(eng, raw)
    eng.close()


# ---- 2. every bucket

_BITS = [LVL_L1, LVL_LFB, LVL_L2, LVL_L3, LVL_LOC_RAM, LVL_REM_RAM1, LVL_REM_RAM2, LVL_REM_CCE1, LVL_REM_CCE2,
         LVL_IO, LVL_UNC]
ALL_LEVELS = ([LVL_HIT | b for b in _BITS] + [LVL_MISS | b for b in _BITS]
              + [LVL_HIT | LVL_MISS | b for b in _BITS]  # HIT beats MISS (quirk Q12)
              + [LVL_NA, LVL_NA | LVL_HIT | LVL_L3, LVL_NA | LVL_MISS | LVL_LOC_RAM, LVL_NA | LVL_L1]
              + [LVL_HIT | LVL_REM_RAM1 | LVL_REM_RAM2, LVL_MISS | LVL_REM_RAM1 | LVL_REM_RAM2,
                 LVL_HIT | LVL_REM_CCE1 | LVL_REM_CCE2, LVL_MISS | LVL_REM_CCE1 | LVL_REM_CCE2]
              + [LVL_HIT | LVL_L1 | LVL_L2 | LVL_IO, LVL_MISS | LVL_L3 | LVL_UNC | LVL_LFB]  # several groups at once
              + [LVL_L2, LVL_IO | LVL_UNC]  # a level without HIT or MISS: no bucket
              + [0])


def _set_levels(rp, seed):
    """Overwrite data_src.mem_lvl of every record with a draw from ALL_LEVELS
    (the generator's mix has single-bit levels only)."""
    rng = np.random.default_rng(seed)
    lv = np.array(ALL_LEVELS, dtype=np.uint64)
    keep = ~np.uint64(0x3FFF << 5)
    for rec in _samples(rp):
        pick = lv[rng.integers(0, lv.shape[0], rec.shape[0])]
        rec["data_src"] = (rec["data_src"] & keep) | (pick << np.uint64(5))


@pytest.fixture(scope="module")
def bucket_case(tmp_path_factory):
    rp = generate(SynthConfig(nb_samples=60_000, nb_intervals=1_500, seed=92))
    _set_levels(rp, 92)
    raw = _oracle(rp, str(tmp_path_factory.mktemp("buckets")))
    tot = _levels(raw).sum(axis=0)  # [2][37]
    assert tot[0].all()  # reads: na_miss and every bucket's count and weight sum
    assert tot[1, 0] and tot[1, 1::2].all()  # writes (weight 0): na_miss and every count
    return rp, raw


@pytest.mark.parametrize("extra", ROUTE_VARIANTS, ids=ROUTE_IDS)
def test_levels_every_bucket(bucket_case, extra):
    rp, raw = bucket_case
    eng = _run_resident(rp, LEVELS | extra)
    assert eng.route_count() > 0
    _check_all(eng, raw)
    eng.close()


# ---- 3. escaped compact records and large weights

@pytest.fixture(scope="module")
def escape_case(tmp_path_factory):
    rp = generate(SynthConfig(nb_samples=60_000, nb_intervals=1_500, seed=93))
    _set_levels(rp, 93)
    rng = np.random.default_rng(93)
    # the compact record's weight field is 11 to 16 bits wide (XLayout::wbits):
    # around every possible escape value 2^wbits - 1; and around the packed LDS
    # counters' limit, kLaneMaxWeight = 2^23
    wesc = [w for b in range(11, 17) for w in ((1 << b) - 2, (1 << b) - 1, 1 << b)]
    wbig = [(1 << 23) - 1, 1 << 23, (1 << 23) + 5, 1 << 30, 1 << 40]
    nesc = nbig = nearly = 0
    for rec in _samples(rp):
        u = rng.random(rec.shape[0])
        esc, big, early = u < 0.01, (u >= 0.01) & (u < 0.012), (u >= 0.012) & (u < 0.02)
        rec["weight"][esc] = rng.choice(np.array(wesc, dtype=np.uint64), int(esc.sum()))
        rec["weight"][big] = rng.choice(np.array(wbig, dtype=np.uint64), int(big.sum()))
        rec["timestamp"][early] = rng.integers(1, T0, int(early.sum()), dtype=np.uint64)  # below tbase
        nesc, nbig, nearly = nesc + int(esc.sum()), nbig + int(big.sum()), nearly + int(early.sum())
    assert nesc > 300 and nbig > 50 and nearly > 300
    raw = _oracle(rp, str(tmp_path_factory.mktemp("escapes")))
    assert int(raw.count_weight[:, :, 1].max()) >= 1 << 23  # a large weight matched
    return rp, raw


@pytest.mark.parametrize("extra", ROUTE_VARIANTS, ids=ROUTE_IDS)
def test_levels_escapes_and_large_weights(escape_case, extra):
    rp, raw = escape_case
    eng = _run_resident(rp, LEVELS | extra)
    assert eng.route_count() > 0
    _check_all(eng, raw)
    eng.close()


# ---- 4. accumulation

def test_levels_accumulate(parity_case):
    """analyze, analyze, synchronize, analyze: three times the oracle's levels
    (the level rows always take atomics; the count and weight rows' first
    flush after a reset stores without reading); reset and one analysis: the
    oracle's."""
    rp, raw = parity_case
    eng = _run_resident(rp, LEVELS)  # (first analysis, synchronised)
    eng.reset()
    eng.analyze()
    eng.analyze()
    eng.synchronize()
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() == 4
    assert np.array_equal(eng.object_levels(), 3 * _levels(raw))
    assert np.array_equal(eng.object_counters()[1], 3 * raw.count_weight)
    _, ns, nf = eng.global_counters()
    assert (ns, nf) == (3 * raw.nb_samples, 3 * raw.nb_found)
    eng.reset()
    eng.analyze()
    eng.synchronize()
    _check_all(eng, raw)
    eng.close()


# ---- 5. streaming with levels

def test_levels_streamed_chunks(parity_case):
    from numamma_amd.engine import Engine

    rp, raw = parity_case
    eng = Engine(flags=LEVELS, nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.stream_begin(chunk_bytes=2 << 20, copy_threads=2)  # 8 MB of records: four chunks
    for r, a, data in rp.linear_buffers():
        eng.submit_buffer(data, r, a)
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    assert eng.route_count() >= 3
    _check_all(eng, raw)
    eng.close()


def test_streaming_with_sample_matches_stays_rejected():
    from numamma_amd.engine import Engine

    eng = Engine(flags=DUMPS)
    with pytest.raises(_lib.NmgError) as ei:
        eng.stream_begin()
    assert ei.value.code == -6  # NMG_ERR_STATE
    eng.close()


# ---- 6. online tables with levels: the id map on the level rows

def test_levels_online_live_tables(tmp_path):
    """A live host's alarm tables (ids in creation order, a permutation of the
    table positions; more than 1023 keys from the second alarm on) streamed
    with levels, against the oracle's alarm mode."""
    from numamma_amd.engine import Engine, table_objects
    from numamma_amd.replay import ObjectTable

    rp = generate(SynthConfig(nb_samples=120_000, nb_intervals=8_000, nb_threads=4, with_stack=False, reuse_frac=0.2,
                              realloc_frac=0.05, buffer_records=500, seed=94))
    rp.buffers.reverse()  # online: oldest ring first
    final = rp.table
    snaps = [(be,) + table_at(final, t) for be, t in online_alarms(rp, 5)]
    assert snaps[-1][1].shape[0] > 1023
    raw = _oracle(rp, str(tmp_path), alarms=snaps)
    assert raw.nb_found > 0 and _levels(raw).sum() > 0

    ent = final.entries
    order = np.lexsort((np.arange(final.nb_entries), ent["alloc_date"]))
    cid = np.empty(final.nb_entries, dtype=np.uint32)  # creation-order id of each table position
    cid[order] = np.arange(final.nb_entries, dtype=np.uint32)
    assert not np.array_equal(cid, np.arange(final.nb_entries))

    def objs(ent4):
        o = np.zeros(ent4.shape[0], dtype=[("a", "<u8"), ("s", "<u8"), ("al", "<u8"), ("fr", "<u8")])
        o["a"], o["s"], o["al"], o["fr"] = ent4[:, 0], ent4[:, 1], ent4[:, 2], ent4[:, 3]
        return o

    eng = Engine(flags=LEVELS, nb_threads=rp.nb_threads)
    eng.set_objects(ObjectTable.empty())
    eng.stream_begin(chunk_bytes=256 << 10, copy_threads=2)
    b0 = 0
    for be, keys, off, ids, ent4 in snaps:
        eng.update_objects(keys, off, cid[ids], objs(ent4))
        for b in rp.buffers[b0:be]:
            eng.submit_ring(b.ring, b.data_tail, b.data_head, b.thread_rank, b.access_type)
        b0 = be
    eng.analyze()
    eng.stream_end()
    eng.synchronize()
    assert eng.route_count() > 0
    eng.update_objects(final.keys, final.entry_off, cid, table_objects(final))  # ma_finalize's table
    eng.table = final
    _check_all(eng, raw, idmap=cid)
    eng.close()


# ---- 7. dump modes on a large table

MAPS = ("00400000-00452000 r-xp 00000000 08:02 173521 /usr/bin/app\n"
        "555500000000-555600000000 rw-p 00000000 00:00 0 [heap]\n"
        "7ffd0000-7ffd1000 rw-p 00000000 00:00 0 [stack]\n")
DUMP_MODULES = [(0x400000, 0x480000, 0x400000, "/usr/bin/app"), (0x480000, 0x4F0000, 0x470000, "/usr/lib/libfoo.so.1")]
DUMP_ALL = _lib.NMG_DUMP_CALLSITES | _lib.NMG_DUMP_ALL | _lib.NMG_DUMP_UNMATCHED


def _same_dirs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.fixture(scope="module")
def dump_case(tmp_path_factory):
    """A large table's replay and a second, shorter buffer set (every other
    buffer: other records at the first set's arena positions), each with the
    oracle's dump files."""
    d = str(tmp_path_factory.mktemp("dumps"))
    rp = generate(SynthConfig(nb_samples=40_000, nb_intervals=3_000, lost_frac=2e-3, wrap_one=True, seed=95))
    rp2 = dataclasses.replace(rp, buffers=rp.buffers[1::2])
    kw = dict(dump=True, dump_all=True, dump_unmatched=True, maps_path="/proc/4242/maps", maps_text=MAPS,
              modules=DUMP_MODULES)
    _oracle(rp, os.path.join(d, "a"), **kw)
    _oracle(rp2, os.path.join(d, "b"), **kw)
    assert any(n.startswith("callsite_summary_") for n in os.listdir(os.path.join(d, "a", "oracle")))
    return d, rp, rp2


@pytest.mark.parametrize("resident,extra", [(False, 0), (True, 0), (False, TINY_POOL), (True, TINY_POOL)],
                         ids=["staged", "resident", "staged_tinypool", "resident_tinypool"])
def test_dump_modes_on_route_path(tmp_path, dump_case, resident, extra):
    """Every dump file byte-identical to the oracle's on the partition-first
    path; then a second analysis of a shorter buffer set on the same engine:
    the per-sample matches of the first one must not show through (records
    the route pass never routes are not written by the kernels)."""
    import torch
    from numamma_amd.engine import Engine

    d, rpa, rpb = dump_case
    eng = Engine(flags=DUMPS | extra, nb_threads=rpa.nb_threads)
    eng.set_objects(rpa.table)
    keep = []
    for tag, rp in (("a", rpa), ("b", rpb)):
        if tag == "b":
            eng.reset()
            eng.clear_buffers()
        if resident:
            arena, offs, lens, ranks, acc = rp.packed()
            keep.append(torch.from_numpy(arena).cuda())
            eng.set_device_buffers(keep[-1].data_ptr(), offs, lens, ranks, acc)
        else:
            eng.submit_replay(rp)
        eng.analyze()
        eng.synchronize()
        assert eng.route_count() == (1 if tag == "a" else 2)
        edir = os.path.join(str(tmp_path), "engine_" + tag)
        eng.report(edir, os.path.join(str(tmp_path), tag + ".txt"), dump_flags=DUMP_ALL, maps_path="/proc/4242/maps",
                   maps_text=MAPS, modules=DUMP_MODULES)
        assert open(os.path.join(d, tag, "o.txt"), "rb").read() == \
            open(os.path.join(str(tmp_path), tag + ".txt"), "rb").read()
        _same_dirs(os.path.join(d, tag, "oracle"), edir)
    eng.close()


# ---- 8. two workers on one device

def test_levels_two_workers(parity_case):
    from numamma_amd.engine import Engine

    rp, raw = parity_case
    eng = Engine(flags=LEVELS, nb_threads=rp.nb_threads, devices=[0, 0])
    eng.set_objects(rp.table)
    eng.submit_replay(rp)
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() >= 2  # both workers' shards took the partition-first path
    _check_all(eng, raw)
    eng.close()
