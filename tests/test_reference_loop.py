"""Pin the oracle against the reference's own sample loop.

The reference's src/mem_sampling.c and src/mem_analyzer.c are compiled
unchanged into oracle/_ref/libref_loop.so (oracle/Makefile,
oracle/ref_loop_shim.c).  These tests drive update_counters, __copy_buffer +
__analyze_buffer (and through them __match_sample), the dated lookup
ma_find_mem_info_from_sample and ma_get_block on crafted inputs, and hold the
oracle (oracle/nmg_oracle.c), which restates them, to the same bytes.  The
recorded vectors under tests/golden/ref_loop are regenerated from the
reference and compared, so they cannot drift; the oracle must reproduce them
(that test needs no reference build).

Not fed to the reference: a SAMPLE record cut by the buffer's end.  It reads
past its copy of the buffer there (mem_sampling.c:865-879), so there is no
defined result to compare with (known divergences)."""
import dataclasses
import os

import numpy as np
import pytest

import pyoracle
import ref_loop_cases as rc
import stream_grammar as sg
from numamma_amd.replay import ENTRY_DTYPE, MEM_DYNAMIC, MEM_STACK, RECORD_DTYPE, STACK_BASE, STACK_END, Buffer, \
    ObjectTable, Replay

needs_ref = pytest.mark.skipif(not pyoracle.ref_loop_available(),
                               reason="reference sample loop (oracle/_ref/libref_loop.so) not built")

CASE_SIZES = [(c, s) for c in rc.CASES for s in rc.SIZES]


# ---------------------------------------------------------------------------
# a. level buckets

def _data_src(lvl, rng):
    """mem_lvl (14 bits at bit 5) with noise in mem_op below and in snoop / lock / tlb / the rest above."""
    n = lvl.shape[0]
    return (lvl << np.uint64(5)) | rng.integers(0, 32, n, dtype=np.uint64) | \
        (rng.integers(0, 1 << 45, n, dtype=np.uint64) << np.uint64(19))


@needs_ref
@pytest.mark.parametrize("access", [0, 1])
@pytest.mark.parametrize("weight", rc.LEVEL_WEIGHTS)
def test_level_buckets_exhaustive(access, weight):
    """All 16 384 mem_lvl values, each on freshly initialised counters: the
    reference's struct mem_counters[2] after update_counters equals the
    oracle's byte for byte (the pair: the other access stays untouched)."""
    rng = np.random.default_rng(weight % 1000 + access)
    ds = _data_src(np.arange(1 << 14, dtype=np.uint64), rng)
    w = np.full(1 << 14, weight, dtype=np.uint64)
    ref = pyoracle.ref_update_counters(ds, w, access)
    ours = pyoracle.update_counters(ds, w, access)
    assert ref.shape == (1 << 14, 2 * pyoracle.COUNTERS_BYTES)
    words = ref.view("<u8").reshape(1 << 14, 2, 75)
    assert np.all(words[:, access, 0] == 1) and np.all(words[:, access, 1] == np.uint64(weight))
    assert np.all(words[:, 1 - access, 0] == 0)
    bad = np.flatnonzero(np.any(ref != ours, axis=1))
    assert bad.size == 0, f"mem_lvl {bad[:8].tolist()} differ"


@needs_ref
@pytest.mark.parametrize("access", [0, 1])
def test_level_buckets_accumulated(access):
    """Every (mem_lvl, weight) pair of the exhaustive test, shuffled, into one
    pair of counters: minima, maxima and the wrapping u64 sums."""
    rng = np.random.default_rng(5 + access)
    lvl = np.repeat(np.arange(1 << 14, dtype=np.uint64), len(rc.LEVEL_WEIGHTS))
    w = np.tile(np.array(rc.LEVEL_WEIGHTS, dtype=np.uint64), 1 << 14)
    p = rng.permutation(lvl.shape[0])
    ds = _data_src(lvl[p], rng)
    ref = pyoracle.ref_update_counters(ds, w[p], access, fresh=False)
    ours = pyoracle.update_counters(ds, w[p], access, fresh=False)
    assert np.array_equal(ref, ours)
    assert int(ref.view("<u8")[0, 75 * access]) == lvl.shape[0]


# ---------------------------------------------------------------------------
# b. record walk

def _compare_replay(rp, tmp_path):
    ref = rc.from_reference(rp)
    ours = rc.from_oracle(rp, str(tmp_path))
    rc.assert_same(ours, ref)
    return ref


@needs_ref
def test_record_walk_every_stream(tmp_path):
    """Every pattern of stream_grammar.py (LOST, header-only and 65,528 B
    records, SAMPLEs of 16 to 104 B, a header whose size passes the end, an
    empty ring, a ring cut inside a SAMPLE): samples seen and found per
    buffer, both global counters, every object's counters and page cells."""
    rp = rc.replay("streams", "small")
    ref = _compare_replay(rp, tmp_path)
    want = [len(sg.walk(b.linear())[0]) for b in rp.buffers if b.linear().shape[0]]
    assert ref["buf_samples"].tolist() == want  # (the referee's count as well)
    assert len(want) == len(rp.buffers) - 1     # (the empty ring gets no index)


def _wrap_at(b, cut, stale=64):
    lin = b.linear()
    first, second = lin[:cut], lin[cut:]
    ring = np.concatenate([second, np.full(stale, 0xAB, dtype=np.uint8), first])
    return Buffer(b.thread_rank, b.access_type, ring, second.shape[0] + stale, second.shape[0])


def _wrap_cuts(lin):
    """Cut offsets by class: where the ring's end falls relative to a record."""
    data = bytes(lin)
    recs, cur = [], 0
    while cur < len(data):
        type_, size = int.from_bytes(data[cur:cur + 4], "little"), int.from_bytes(data[cur + 6:cur + 8], "little")
        recs.append((cur, type_, size))
        cur += size
    cuts = {}
    for name, pred in (("sample40", lambda t, s: t == sg.SAMPLE and s == 40),
                       ("sample16", lambda t, s: t == sg.SAMPLE and s == 16),
                       ("sample_long", lambda t, s: t == sg.SAMPLE and s > 40),
                       ("other", lambda t, s: t != sg.SAMPLE and s >= 24)):
        hit = [r for r in recs[2:-2] if pred(r[1], r[2])]
        if not hit:
            continue
        o, _, s = hit[len(hit) // 2]
        cuts[name + ":boundary"] = o
        cuts[name + ":header"] = o + 4
        cuts[name + ":after_header"] = o + 8
        if s > 16:
            cuts[name + ":body"] = o + 16
        cuts[name + ":last_byte"] = o + s - 1
    return cuts


@needs_ref
def test_record_walk_wrapped_rings(tmp_path):
    """Rings wrapped at every offset class -- on a record boundary, inside a
    header, right after it, inside the body and one byte before the end -- of
    40 B, 16 B-header and long SAMPLEs and of other records."""
    rp = rc.replay("streams", "small")
    where = rp.meta["patterns"]
    bufs, classes = [], set()
    for pat in ("dense", "short", "long", "alternate"):
        b = rp.buffers[where[pat][0]]
        for name, cut in _wrap_cuts(b.linear()).items():
            bufs.append(_wrap_at(b, cut, stale=8 if len(bufs) % 2 else 64))
            classes.add(name)
    assert {"sample40:header", "sample16:boundary", "sample16:header", "sample_long:body", "other:body",
            "sample40:last_byte"} <= classes
    wrapped = dataclasses.replace(rp, buffers=bufs)
    ref = _compare_replay(wrapped, tmp_path)
    # a wrapped ring holds what its linear twin holds
    lin = [len(sg.walk(b.linear())[0]) for b in bufs]
    assert ref["buf_samples"].tolist() == lin and min(lin) > 100


def _one_buffer(rp, raw):
    raw = np.frombuffer(raw, dtype=np.uint8).copy()
    return dataclasses.replace(rp, buffers=[Buffer(1, 0, raw, 0, raw.shape[0])])


@needs_ref
@pytest.mark.parametrize("k", [1, 7, 200])
def test_record_walk_stops_on_size_zero(tmp_path, k):
    """A header of size 0 behind k SAMPLEs: the reference counts the k samples
    and calls abort() (mem_sampling.c:857-860); the oracle refuses the replay
    with its size-0 error."""
    rp = rc.replay("sweep", "small")  # (pure 40 B records: a pool of sample payloads)
    pool, rng = sg.Pool(rp), np.random.default_rng(k)
    one = _one_buffer(rp, b"".join(sg.regular(pool, k) + [sg.header(sg.LOST, 0)] + sg.regular(pool, 5)))
    ref = pyoracle.RefLoop()
    ref.add_table(one.table)
    b = one.buffers[0]
    st, ns, _ = ref.feed(b.ring, b.data_tail, b.data_head, b.thread_rank, b.access_type)
    assert (st, ns) == (pyoracle.RL_ABORT, k)
    assert int(ref.global_counters()[0].view("<u8")[0]) == k
    with pytest.raises(RuntimeError, match="size 0"):
        rc.from_oracle(one, str(tmp_path))


@needs_ref
def test_record_walk_unaligned_sizes(tmp_path):
    """Record sizes that are no multiple of 8 (12, 20, 44): the reference has
    no rule against them and walks on by the size; so does the oracle (the
    engine alone refuses them, NMG_ERR_UNALIGNED)."""
    rp = rc.replay("sweep", "small")
    pool, rng = sg.Pool(rp), np.random.default_rng(3)
    parts = []
    for size in (12, 20, 44, 12, 12):
        parts += sg.regular(pool, 9) + [sg.header(sg.LOST, size) + rng.bytes(size - 8)]
    one = _one_buffer(rp, b"".join(parts + sg.regular(pool, 2)))
    ref = _compare_replay(one, tmp_path)
    assert ref["buf_samples"].tolist() == [47]


# ---------------------------------------------------------------------------
# c. dated lookup

@needs_ref
@pytest.mark.parametrize("nkeys", [1, 2, 1025])
def test_dated_lookup_edges(nkeys):
    """ma_find_mem_info_from_sample on every boundary of every entry (the key,
    key - 1, the first byte, end - 1, end; the alloc and free dates and one
    tick outside; addresses 0, 2^63 and 2^64 - 1), chains of three entries on
    reused keys and realloc'd objects: the oracle's lookup names the same
    object for every sample."""
    rp = rc.edge_replay(nkeys)
    tab = rp.table
    chain = np.diff(tab.entry_off.astype(np.int64))
    key_of = np.repeat(tab.keys, chain)
    if nkeys > 2:
        assert chain.max() == 3 and np.any(tab.entries["buffer_addr"] != key_of)
    ref = pyoracle.RefLoop()
    obj = ref.add_table(tab)
    entry_of = np.full(int(obj.max()) + 2, -1, dtype=np.int64)
    entry_of[obj] = np.arange(obj.shape[0])
    addr, ts = rc.edge_samples(tab, None)
    got = entry_of[ref.find(addr, ts)]  # (-1 indexes the spare last slot: no match)
    e = tab.entries
    ent4 = np.stack([e["buffer_addr"], e["buffer_size"], e["alloc_date"], e["free_date"]], axis=1)
    ours = np.array([pyoracle.lookup(tab.keys, tab.entry_off, ent4, int(a), int(t)) for a, t in zip(addr, ts)])
    bad = np.flatnonzero(got != ours)
    assert bad.size == 0, [(hex(int(addr[i])), int(ts[i]), int(got[i]), int(ours[i])) for i in bad[:5]]
    assert (got >= 0).sum() >= 6 * nkeys and (got < 0).sum() >= 6 * nkeys


# ---------------------------------------------------------------------------
# d. page index

HUGE = 4  # entry of _page_replay's 64 TiB object


def _page_replay():
    """Objects of 1, 2 and 65 pages, the [stack] and a 64 TiB mapping; samples
    on the first and last byte of pages, from three threads; on the [stack]
    (timestamp 0: the only one its dates 0..0 let through) up to its last page,
    0x5ffffff; on the mapping at offsets whose page number passes 2^31 and
    2^32, which ma_get_block's `int page_no` truncates."""
    sizes = (4096, 8192, 65 * 4096)
    ent = np.zeros(5, dtype=ENTRY_DTYPE)
    keys = np.array([0x10000000, 0x20000000, 0x30000000, STACK_BASE, 1 << 47], dtype=np.uint64)
    ent["buffer_addr"] = keys
    ent["buffer_size"][:3], ent["buffer_size"][3], ent["buffer_size"][HUGE] = sizes, STACK_END - STACK_BASE, 1 << 46
    ent["initial_buffer_size"] = ent["buffer_size"]
    ent["alloc_date"], ent["free_date"] = 10, 1000
    ent["alloc_date"][3] = ent["free_date"][3] = 0
    ent["mem_type"], ent["mem_type"][3] = MEM_DYNAMIC, MEM_STACK
    ent["caller_rip"], ent["id"] = 0x1000, np.arange(1, 6)
    strings = b"app.c:1(f)\0[stack]\0"
    ent["caller_off"][3] = 11
    tab = ObjectTable(keys, np.arange(6, dtype=np.uint32), ent, np.zeros(0, dtype=np.uint64), strings)
    addr, ts, want = [], [], []

    def hit(e, off, t):
        addr.append(int(keys[e]) + off), ts.append(t), want.append((e, (off // 4096) & 0xFFFFFFFF))

    for i, size in enumerate(sizes):
        for off in sorted({0, 1, 4095, size - 1, size // 2, max(size - 4096, 0), max(size - 4097, 0)}):
            hit(i, off, 500)
    stack_size = STACK_END - STACK_BASE
    for off in (0, 4095, 4096, 0x1234567 * 4096 + 9, stack_size - 4096, stack_size - 1):
        hit(3, off, 0)
    for page in (0, 2**31 - 1, 2**31, 2**31 + 5, 2**32 - 1, 2**32, 2**32 + 7, 2**34 - 1):
        for off in (page * 4096, page * 4096 + 4095):
            hit(HUGE, off, 500)
    rec = np.zeros(len(addr), dtype=RECORD_DTYPE)
    rec["type"], rec["misc"], rec["size"] = 9, 2, 40
    rec["addr"], rec["timestamp"] = np.array(addr, dtype=np.uint64), np.array(ts, dtype=np.uint64)
    rec["weight"], rec["data_src"] = 7, np.uint64(0x42) << np.uint64(5)
    bufs = [Buffer(t, t % 2, np.frombuffer(rec.tobytes(), dtype=np.uint8).copy(), 0, rec.nbytes) for t in (0, 2, 5)]
    return Replay(8, tab, bufs), want


@needs_ref
def test_page_index(tmp_path):
    """Page counts per (object, thread, page): the reference's blocks equal the
    oracle's cells and the counts worked out from `int page_no = offset / 4096`."""
    rp, want = _page_replay()
    ref = _compare_replay(rp, tmp_path)
    cells = {}
    for t in (0, 2, 5):
        for e, page in want:
            cells[e, t, page] = cells.get((e, t, page), 0) + 1
    expect = rc.sort_cells(np.array([k + (v,) for k, v in cells.items()], dtype=np.uint32))
    assert np.array_equal(ref["cells"], expect)
    assert int(ref["totals"][1]) == 3 * len(want)
    pages = ref["cells"][:, 2]
    assert 0x5FFFFFF in pages[ref["cells"][:, 0] == 3].tolist()
    assert {0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 7} <= set(pages[ref["cells"][:, 0] == HUGE].tolist())


# ---------------------------------------------------------------------------
# the recorded vectors

@needs_ref
@pytest.mark.parametrize("case,size", CASE_SIZES)
def test_vectors_are_the_references(case, size):
    """tests/golden/ref_loop/<case>_<size>.npz is what the reference returns today."""
    rc.assert_same(rc.from_reference(rc.replay(case, size)), rc.load_golden(case, size))


@pytest.mark.parametrize("case,size", CASE_SIZES)
def test_oracle_reproduces_vectors(tmp_path, case, size):
    rc.assert_same(rc.from_oracle(rc.replay(case, size), str(tmp_path)), rc.load_golden(case, size))


def test_vector_replays_have_their_shape():
    """What the GPU tests rely on: table sizes on either side of the 1023-key
    threshold, every level once per access, chains and realloc'd objects."""
    for case in rc.CASES:
        small, large = rc.replay(case, "small"), rc.replay(case, "large")
        assert small.table.nb_keys == 40 and large.table.nb_keys == 40 + rc.NB_FILLERS > 1023
        assert [b.ring.tobytes() for b in small.buffers] == [b.ring.tobytes() for b in large.buffers]
        g = rc.load_golden(case, "small")
        assert 20_000 < int(g["totals"][0]) <= 70_000 and 0 < int(g["totals"][1]) < int(g["totals"][0])
        assert os.path.getsize(rc.golden_path(case, "large")) < 256 * 1024
    sweep = rc.replay("sweep", "small")
    rec = np.concatenate([b.ring.view(RECORD_DTYPE) for b in sweep.buffers])
    acc = np.concatenate([np.full(b.ring.shape[0] // 40, b.access_type) for b in sweep.buffers])
    lvl = (rec["data_src"] >> np.uint64(5)) & np.uint64(0x3FFF)
    for a in (0, 1):
        assert np.array_equal(np.sort(lvl[acc == a]), np.arange(1 << 14, dtype=np.uint64))
    assert sweep.table.nb_entries == 64 and {b.thread_rank for b in sweep.buffers} == set(range(8))
    edges = rc.replay("edges", "small").table
    assert np.diff(edges.entry_off.astype(np.int64)).max() == 3
    assert np.any(edges.entries["buffer_addr"] != np.repeat(edges.keys, np.diff(edges.entry_off.astype(np.int64))))
