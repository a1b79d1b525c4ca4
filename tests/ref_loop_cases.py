"""Replays whose results the reference's own sample loop recorded
(tests/golden/ref_loop/*.npz), and the glue that turns a run of the reference
(pyoracle.RefLoop), of the oracle (a raw-results dump) or of the engine into
the same arrays (shared by test_reference_loop.py and
test_gpu_reference_vectors.py; not a test module).

Building a replay needs numpy only.  Three replays, each at two table sizes
(40 keys: attribute_kernel's LDS tree; the same objects plus 1000 filler keys
that no sample can match, 1040 keys: the partition-first path):

* sweep: every mem_lvl value (16 384) once per access type, over 64 objects
  (40 keys, 24 of them reused) and 8 threads, the weights of the level test
  among small ones, noise in the other data_src bits;
* streams: every pattern of stream_grammar.py except tiny (about 22k samples
  in about 3 MB of irregular records);
* edges: samples on every lookup boundary of a table with chains of three
  entries per reused key and realloc'd objects.

The arrays of a result (dict):
  global       u64[2][75]  struct mem_counters x {read, write}, as words
  totals       u64[2]      samples, found
  buf_samples  u32[B]      per non-empty buffer
  buf_found    u32[B]
  entries      u64[E][78]  per entry and access: count, weight, N/A, 18 x (count, sum)
  cells        u32[n][4]   (entry, thread, page, read + write count), sorted, non-zero
"""
import dataclasses
import os

import numpy as np

import stream_grammar as sg
from numamma_amd.replay import (ENTRY_DTYPE, MEM_DYNAMIC, RECORD_DTYPE, Buffer, ObjectTable, Replay, SynthConfig,
                                generate)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_loop")
NB_FILLERS = 1000
COUNTER_WORDS = 75  # struct mem_counters: 3 + 18 x (count, min, max, sum)
SUM_WORDS = 39      # count, weight, N/A, 18 x (count, sum)
# of a struct mem_counters' 75 words, the 39 that add up across blocks
SUM_OF_COUNTER = np.array([0, 1, 2] + [3 + 4 * b + j for b in range(18) for j in (0, 3)])
LEVEL_WEIGHTS = (0, 1, 1 << 23, (1 << 31) - 1, 1 << 31, (1 << 32) + 3, 1 << 63)
KEYS = ("global", "totals", "buf_samples", "buf_found", "entries", "cells")


# ---------------------------------------------------------------------------
# tables

def with_fillers(rp, n=NB_FILLERS):
    """rp over the same objects plus n filler keys: 16 B objects that lived
    from date 1 to date 2 (the replays' dates are 0 or about 10^12), half of
    them below the lowest key, half between the heap and the [stack].  A
    filler can only become the lower-bound node of a sample that had none."""
    t = rp.table
    lo = np.uint64(0x100000000) + np.arange(n // 2, dtype=np.uint64) * np.uint64(64)
    hi = np.uint64(0x600000000000) + np.arange(n - n // 2, dtype=np.uint64) * np.uint64(64)
    fk = np.concatenate([lo, hi])
    assert not np.intersect1d(fk, t.keys).size
    fe = np.zeros(n, dtype=ENTRY_DTYPE)
    fe["buffer_addr"], fe["buffer_size"], fe["initial_buffer_size"] = fk, 16, 16
    fe["alloc_date"], fe["free_date"] = 1, 2
    fe["caller_rip"], fe["mem_type"] = 0x555555550000, MEM_DYNAMIC
    heap = np.flatnonzero(t.entries["mem_type"] == MEM_DYNAMIC)
    fe["caller_off"] = t.entries["caller_off"][heap[0]]
    keys = np.concatenate([t.keys, fk])
    counts = np.concatenate([np.diff(t.entry_off.astype(np.int64)), np.ones(n, dtype=np.int64)])
    first = np.concatenate([t.entry_off[:-1].astype(np.int64), t.nb_entries + np.arange(n)])
    ent = np.concatenate([t.entries, fe])
    order = np.argsort(keys, kind="stable")
    pick = np.concatenate([np.arange(first[k], first[k] + counts[k]) for k in order])
    ent = ent[pick].copy()
    ent["id"] = np.arange(1, ent.shape[0] + 1)
    off = np.zeros(keys.shape[0] + 1, dtype=np.uint32)
    off[1:] = np.cumsum(counts[order])
    return dataclasses.replace(rp, table=ObjectTable(keys[order], off, ent, t.callstack_pool, t.string_pool))


def _cut_table(rp, nkeys):
    t = rp.table
    assert t.nb_keys >= nkeys
    ne = int(t.entry_off[nkeys])
    return ObjectTable(t.keys[:nkeys].copy(), t.entry_off[:nkeys + 1].copy(), t.entries[:ne].copy(),
                       t.callstack_pool, t.string_pool)


def _buffers(rec, per, threads, rng, access=None):
    out = []
    for i, s in enumerate(range(0, rec.shape[0], per)):
        raw = np.frombuffer(rec[s:s + per].tobytes(), dtype=np.uint8).copy()
        out.append(Buffer(i % threads, int(rng.integers(0, 2)) if access is None else access, raw, 0, raw.shape[0]))
    return out


# ---------------------------------------------------------------------------
# the three replays

def sweep_replay():
    """40 heap keys, 24 of them reused once (64 entries), sizes 1 B to 3 pages
    (odd ones among them); 16 buffers, one per (thread, access), 2048 records
    each.  One sample in 16 falls in the gap after its object."""
    src = generate(SynthConfig(nb_samples=64, nb_intervals=40, nb_globals=0, with_stack=False, reuse_frac=1.0,
                               size_min=1, size_max=3 * 4096, seed=401))
    t = src.table
    assert t.nb_keys == 40 and t.nb_entries == 80
    keep = np.ones(80, dtype=bool)
    keep[2 * np.arange(16) + 1] = False  # the first 16 keys lose their older entry
    off = np.zeros(41, dtype=np.uint32)
    off[1:] = np.cumsum(np.where(np.arange(40) < 16, 1, 2))
    tab = ObjectTable(t.keys, off, t.entries[keep].copy(), t.callstack_pool, t.string_pool)
    tab.entries["id"] = np.arange(1, 65)
    rng = np.random.default_rng(402)
    ent = tab.entries
    ent["buffer_size"][:3] = (1, 4097, 8191)
    ent["initial_buffer_size"][:3] = ent["buffer_size"][:3]
    lvl = np.tile(np.arange(1 << 14, dtype=np.uint64), 2)
    access = np.repeat(np.arange(2), 1 << 14)
    n = lvl.shape[0]
    e = rng.integers(0, 64, n)
    off = (rng.random(n) * ent["buffer_size"][e]).astype(np.uint64)
    gap = rng.random(n) < 1 / 16
    ts = ent["alloc_date"][e] + ((ent["free_date"][e] - ent["alloc_date"][e]).astype(np.float64) * rng.random(n)).astype(np.uint64)
    w = rng.integers(0, 3000, n).astype(np.uint64)
    special = rng.random(n) < 0.05
    w[special] = np.array(LEVEL_WEIGHTS, dtype=np.uint64)[rng.integers(0, len(LEVEL_WEIGHTS), int(special.sum()))]
    rec = np.zeros(n, dtype=RECORD_DTYPE)
    rec["type"], rec["misc"], rec["size"] = 9, 2, 40
    rec["timestamp"] = ts
    rec["addr"] = ent["buffer_addr"][e] + np.where(gap, ent["buffer_size"][e], off)
    rec["weight"] = w
    noise = rng.integers(0, 1 << 45, n, dtype=np.uint64) << np.uint64(19)
    rec["data_src"] = (lvl << np.uint64(5)) | rng.integers(0, 32, n, dtype=np.uint64) | noise
    bufs = []
    for a in (0, 1):
        r = rec[access == a][rng.permutation(1 << 14)]
        for t in range(8):
            raw = np.frombuffer(r[t * 2048:(t + 1) * 2048].tobytes(), dtype=np.uint8).copy()
            bufs.append(Buffer(t, a, raw, 0, raw.shape[0]))
    return Replay(8, tab, bufs)


def streams_replay():
    """stream_grammar's patterns over 31 heap keys, 8 globals and the [stack]: 40 keys."""
    rp = sg.grammar_replay(31)
    assert rp.table.nb_keys == 40
    return rp


def edge_samples(tab, rng):
    """(addr, ts) on every boundary of every entry of tab: the key, key - 1,
    the first byte, end - 1, end; the alloc and free dates, one tick outside
    each and the middle; then addresses 0, 1, 2^63, 2^64 - 2 and 2^64 - 1."""
    e = tab.entries
    key_of = np.repeat(np.arange(tab.nb_keys), np.diff(tab.entry_off.astype(np.int64)))
    addrs, tss = [], []
    for i in range(e.shape[0]):
        x = e[i]
        key, a = int(tab.keys[key_of[i]]), int(x["buffer_addr"])
        end = a + int(x["buffer_size"])
        al, fr = int(x["alloc_date"]), int(x["free_date"])
        for ad in (key, key - 1, a, end - 1, end):
            for ts in (al, fr, max(al - 1, 0), min(fr + 1, 2**64 - 1), (al + fr) // 2):
                addrs.append(ad % 2**64)
                tss.append(ts)
    for ad in (0, 1, 2**63, 2**64 - 2, 2**64 - 1):
        for ts in (0, 2**64 - 1, int(e["alloc_date"][0])):
            addrs.append(ad)
            tss.append(ts)
    return np.array(addrs, dtype=np.uint64), np.array(tss, dtype=np.uint64)


def edge_replay(nkeys, seed=411, repeat=1):
    """A table of exactly nkeys heap keys with chains of three entries on the
    reused keys and realloc'd objects (key != buffer_addr), and `repeat`
    shuffled copies of edge_samples() with L1-hit levels."""
    src = generate(SynthConfig(nb_samples=64, nb_intervals=nkeys + 50, nb_globals=0, with_stack=False,
                               reuse_frac=0.3, reuse_depth=3, realloc_frac=0.2, seed=seed))
    tab = _cut_table(src, nkeys)
    rng = np.random.default_rng(seed + 1)
    addr, ts = edge_samples(tab, rng)
    addr, ts = np.tile(addr, repeat), np.tile(ts, repeat)
    n = addr.shape[0]
    rec = np.zeros(n, dtype=RECORD_DTYPE)
    rec["type"], rec["misc"], rec["size"] = 9, 2, 40
    rec["timestamp"], rec["addr"] = ts, addr
    rec["weight"] = rng.integers(0, 2000, n)
    rec["data_src"] = np.uint64(0x42) << np.uint64(5)  # L1 hit
    rec = rec[rng.permutation(n)]
    return Replay(src.nb_threads, tab, _buffers(rec, 1500, src.nb_threads, rng))


def edges_replay():
    """40 keys; the boundary set 24 times over (about 36k records)."""
    return edge_replay(40, repeat=24)


CASES = {"sweep": sweep_replay, "streams": streams_replay, "edges": edges_replay}
SIZES = ("small", "large")
_cache = {}


def replay(case, size):
    """The replay of a case at a table size, built once per process."""
    if (case, "small") not in _cache:
        _cache[case, "small"] = CASES[case]()
    if (case, size) not in _cache:
        _cache[case, size] = with_fillers(_cache[case, "small"])
    return _cache[case, size]


def golden_path(case, size):
    return os.path.join(GOLDEN_DIR, f"{case}_{size}.npz")


def load_golden(case, size):
    with np.load(golden_path(case, size)) as z:
        return {k: z[k] for k in KEYS}


# ---------------------------------------------------------------------------
# results as arrays

def sort_cells(cells):
    c = np.asarray(cells, dtype=np.uint32).reshape(-1, 4)
    return c[np.lexsort((c[:, 2], c[:, 1], c[:, 0]))]


def from_reference(rp, match_samples=True):
    """rp through the reference's own loop (pyoracle.RefLoop)."""
    import pyoracle

    ref = pyoracle.RefLoop(match_samples)
    obj = ref.add_table(rp.table)
    for b in rp.buffers:
        st, _, _ = ref.feed(b.ring, b.data_tail, b.data_head, b.thread_rank, b.access_type)
        assert st == pyoracle.RL_OK, st
    g, ns, nf = ref.global_counters()
    E = rp.table.nb_entries
    entries = np.zeros((E, 2 * SUM_WORDS), dtype=np.uint64)
    cells = []
    for e in range(E):
        rows = ref.blocks(int(obj[e]))
        if rows is None or not rows.shape[0]:
            continue
        c = rows[:, 2:].reshape(-1, 2, COUNTER_WORDS)
        entries[e] = c[:, :, SUM_OF_COUNTER].sum(axis=0, dtype=np.uint64).reshape(-1)
        tot = c[:, 0, 0] + c[:, 1, 0]
        cells.append(np.stack([np.full(rows.shape[0], e, dtype=np.uint64), rows[:, 0], rows[:, 1], tot], axis=1))
    cells = np.concatenate(cells).astype(np.uint32) if cells else np.zeros((0, 4), dtype=np.uint32)
    return {"global": g.view("<u8").reshape(2, COUNTER_WORDS).copy(), "totals": np.array([ns, nf], dtype=np.uint64),
            "buf_samples": np.array(ref.buf_samples, dtype=np.uint32),
            "buf_found": np.array(ref.buf_found, dtype=np.uint32), "entries": entries, "cells": sort_cells(cells)}


def from_raw(res):
    """A raw-results dump (numamma_amd.results.RawResults: the oracle's or the engine's)."""
    return {"global": res.global_counters.copy(), "totals": np.array([res.nb_samples, res.nb_found], dtype=np.uint64),
            "buf_samples": res.buf_samples.astype(np.uint32), "buf_found": res.buf_found.astype(np.uint32),
            "entries": res.entries[:, 1:].copy(), "cells": sort_cells(res.cells)}


def from_oracle(rp, d):
    import pyoracle
    from numamma_amd.results import RawResults

    path = os.path.join(d, "replay.bin")
    rp.write(path)
    pyoracle.run(path, os.path.join(d, "oracle"), os.path.join(d, "oracle_stdout.txt"), os.path.join(d, "oracle_raw.bin"))
    return from_raw(RawResults.read(os.path.join(d, "oracle_raw.bin")))


def assert_same(got, want, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{k}: {bad.shape[0]} words differ, first at {bad[0].tolist()}: "
                                 f"{a[tuple(bad[0])]} != {b[tuple(bad[0])]}")


def write_golden():
    """Record what the reference returns (needs oracle/_ref/libref_loop.so)."""
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    for case in CASES:
        for size in SIZES:
            np.savez_compressed(golden_path(case, size), **from_reference(replay(case, size)))


if __name__ == "__main__":  # (with the repository root and oracle/ on PYTHONPATH)
    write_golden()
